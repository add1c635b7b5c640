"""A float64 restatement of the f32 Dense / chain / fused-MLP operators (hip/dense.hip, chain_device.inc, mlp_device.inc), from numpy alone,
with the inputs on which a correct fp32 kernel has exactly one right answer and the error bound every other input is held to.  A helper
module (tests/test_dense_ref.py checks it without a GPU, tests/test_dense_exact_gpu.py uses it on one), not a conftest.

Layers are (W [K, M] f32, b [M] f32 or None); `acts` names what follows each layer ("", "Relu", "Sigmoid", "Tanh", "LeakyRelu" with
alpha = f32(0.1)); `head` is "", "Softmax", "LogSoftmax" or "ArgMax" (ties to the lower index: ONNX select_last_index = 0).

The bound (error_bound).  A layer's f32 sum of K products, in ANY order, rounds each product and each partial sum once, each to within
2^-24 of a partial result that never exceeds mag = |x| |W| + |b|; with the bias add and the final rounding that is (K + 2) 2^-24 mag.  The
error e of the layer's input arrives through |W|, so before the activation

    e_l = (K_l + 2) 2^-24 mag_l + |W_l|^T e_(l-1),         mag_l = (|h_(l-1)| + e_(l-1)) |W_l| + |b_l|.

An activation passes it on by its Lipschitz constant (1; Sigmoid 1/4) and adds its own rounding: nothing for Relu, one rounding of the
product for LeakyRelu, 2 ulp of the value (2 * 2^-23 |v|) for Sigmoid and Tanh -- the bound device_common.hpp states for expf / tanhf.
Softmax over M logits with errors <= d: every exp(z_i - max) and their sum move by a factor within e^(+-2d), and expf (2 ulp), the
subtraction, the M - 1 additions and the division round M + 6 times at most, so |dp| <= p (2 d + (M + 6) 2^-24) + 2^-126 (a probability
below the smallest normal f32 may arrive as zero); LogSoftmax is the logarithm of that, |dv| <= 2 d + (M + 6) 2^-24 (1 + |v|)."""
from __future__ import annotations

import math

import numpy as np

from infera_amd import onnx_writer as W

U = 2.0 ** -24
LEAKY = np.float32(0.1)


# ---- weights, reference, bound ----------------------------------------------------------------------------------------------------

def mlp_weights(dims, seed: int = 1234):
    """[(W [K, M], b [M])] of onnx_writer.mlp(dims, seed=seed), draw for draw"""
    ws = W._WeightStream(seed)
    return [(ws.take((k, m), k), ws.take((m,), k)) for k, m in zip(dims[:-1], dims[1:])]


def default_acts(n):
    return ["Relu"] * (n - 1) + [""]


def _act64(z, kind):
    if kind == "Relu":
        return np.maximum(z, 0.0)
    if kind == "Sigmoid":
        with np.errstate(over="ignore"):
            return 1.0 / (1.0 + np.exp(-z))
    if kind == "Tanh":
        return np.tanh(z)
    if kind == "LeakyRelu":
        return np.where(z >= 0, z, np.float64(LEAKY) * z)
    assert kind == "", kind
    return z


def argmax_low(z):
    """the first index of each row's maximum"""
    return np.argmax(z, axis=1)  # (numpy returns the first occurrence)


def forward64(layers, x, acts=None, head: str = ""):
    """{"out": the served values in float64, "pre": each layer's sums, "mag": each layer's |x| |W| + |b|, "logits": what the head reads}"""
    acts = default_acts(len(layers)) if acts is None else list(acts)
    h = np.asarray(x, np.float64)
    pre, mag = [], []
    for (w, b), a in zip(layers, acts):
        w64 = np.asarray(w, np.float64)
        b64 = np.zeros(w64.shape[1]) if b is None else np.asarray(b, np.float64)
        mag.append(np.abs(h) @ np.abs(w64) + np.abs(b64))
        z = h @ w64 + b64
        pre.append(z)
        h = _act64(z, a)
    out = h
    if head == "Softmax" or head == "LogSoftmax":
        s = h - h.max(1, keepdims=True)
        ls = np.log(np.exp(s).sum(1, keepdims=True))
        out = np.exp(s - ls) if head == "Softmax" else s - ls
    elif head == "ArgMax":
        out = argmax_low(h).astype(np.float64)[:, None]
    else:
        assert head == "", head
    return {"out": out, "pre": pre, "mag": mag, "logits": h}


def error_bound(layers, x, acts=None, head: str = ""):
    """(the reference, the bound on |served - reference| per element): the module docstring's derivation"""
    acts = default_acts(len(layers)) if acts is None else list(acts)
    h = np.asarray(x, np.float64)
    e = np.zeros_like(h)
    for (w, b), a in zip(layers, acts):
        aw = np.abs(np.asarray(w, np.float64))
        b64 = np.zeros(aw.shape[1]) if b is None else np.asarray(b, np.float64)
        mag = (np.abs(h) + e) @ aw + np.abs(b64)
        e = (aw.shape[0] + 2) * U * mag + e @ aw
        h = _act64(h @ np.asarray(w, np.float64) + b64, a)
        if a == "Sigmoid":
            e = e / 4 + 4 * U * np.abs(h)
        elif a == "Tanh":
            e = e + 4 * U * np.abs(h)
        elif a == "LeakyRelu":
            e = e + U * np.abs(h)
    ref = forward64(layers, x, acts, head)["out"]
    if head == "Softmax":
        e = ref * (2 * e.max(1, keepdims=True) + (h.shape[1] + 6) * U) + 2.0 ** -126
    elif head == "LogSoftmax":
        e = 2 * e.max(1, keepdims=True) + (h.shape[1] + 6) * U * (1 + np.abs(ref))
    else:
        assert head == "", "a label has no bound: exclude the rows whose deciding gap is below twice the logits' bound"
    return ref, e


# ---- the graphs -------------------------------------------------------------------------------------------------------------------

def graph(layers, acts=None, head: str = "", form: str = "gemm") -> bytes:
    """explicit weights as an ONNX model: `form` gemm / matmul_add / trans_b, as onnx_writer.mlp spells them; the ArgMax head it lacks"""
    acts = default_acts(len(layers)) if acts is None else list(acts)
    nodes, inits, cur = [], [], "X"
    for l, ((w, b), a) in enumerate(zip(layers, acts)):
        w = np.ascontiguousarray(w, np.float32)
        b = np.zeros(w.shape[1], np.float32) if b is None else np.ascontiguousarray(b, np.float32)
        inits += [W.tensor(f"W{l}", np.ascontiguousarray(w.T) if form == "trans_b" else w), W.tensor(f"B{l}", b)]
        if form == "matmul_add":
            nodes += [W.node("MatMul", [cur, f"W{l}"], [f"Z{l}"]), W.node("Add", [f"Z{l}", f"B{l}"], [f"H{l}"])]
        else:
            nodes.append(W.node("Gemm", [cur, f"W{l}", f"B{l}"], [f"H{l}"], [W.attr_i("transB", 1)] if form == "trans_b" else []))
        cur = f"H{l}"
        if a:
            nodes.append(W.node(a, [cur], [f"A{l}"], [W.attr_f("alpha", float(LEAKY))] if a == "LeakyRelu" else []))
            cur = f"A{l}"
    k, m = layers[0][0].shape[0], layers[-1][0].shape[1]
    if head == "ArgMax":
        nodes.append(W.node("ArgMax", [cur], ["Y"], [W.attr_i("axis", 1), W.attr_i("keepdims", 0)]))
        out = W.value_info("Y", ["N"], W.INT64)
    else:
        nodes.append(W.node(head or "Identity", [cur], ["Y"], [W.attr_i("axis", 1)] if head else []))
        out = W.value_info("Y", ["N", m])
    return W.model("dense_ref", nodes, inits, [W.value_info("X", ["N", k])], [out])


# ---- inputs with one right answer -------------------------------------------------------------------------------------------------

def full_mantissa(rng, shape):
    """f32 values whose 24 significand bits are all in use (the lowest one set), exponents in [-20, 20], both signs: far from denormals and
    overflow, and nothing a kernel may drop"""
    sig = rng.integers(1 << 23, 1 << 24, shape) | 1
    v = np.ldexp(sig.astype(np.float64), rng.integers(-20, 21, shape) - 23) * rng.choice([-1.0, 1.0], shape)
    out = v.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), v)
    return out


def selection(rng, K, M):
    """a signed selection K -> M: column m holds one +-2^e, in row (a m + c) mod K, a coprime to K (every k is read once M >= K) and c such that
    the last column reads the last k (the last partial K group and the last output tile meet); no bias"""
    a = next(s for s in (7, 5, 3, 2, 1) if math.gcd(s, K) == 1)
    c = (K - 1 - a * (M - 1)) % K
    w = np.zeros((K, M), np.float32)
    rows = (a * np.arange(M) + c) % K
    w[rows, np.arange(M)] = np.ldexp(rng.choice([-1.0, 1.0], M), rng.integers(-3, 4, M)).astype(np.float32)
    return w, None


def grid_layers(rng, dims, tie_columns: bool = False):
    """integers: the first layer in [-8, 8], later ones in {-1, 0, 1}, biases in [-8, 8]; tie_columns: output m of the last layer repeats
    output M - 1 - m (an odd M's middle one repeats output 0), so every row's largest score is there twice and ArgMax must pick the lower"""
    layers = []
    for l, (k, m) in enumerate(zip(dims[:-1], dims[1:])):
        lim = 8 if l == 0 else 1
        w, b = rng.integers(-lim, lim + 1, (k, m)), rng.integers(-8, 9, m)
        if tie_columns and l == len(dims) - 2:
            src = np.minimum(np.arange(m), m - 1 - np.arange(m))
            if m % 2:
                src[m // 2] = 0
            w, b = w[:, src], b[src]
        layers.append((w.astype(np.float32), b.astype(np.float32)))
    return layers


def exact_case(kind: str, dims, rows: int, seed: int = 0, tie_columns: bool = False):
    """(layers, x) of kind "grid" (a: every term counted once), "select" (b: activations pass through untouched) or "onehot" (c: weights pass
    through untouched); Relu between the layers, nothing after the last.  `rows` rows: a prefix of a longer draw is the same rows."""
    rng = np.random.default_rng([seed, {"grid": 1, "select": 2, "onehot": 3}[kind], *dims])
    K = dims[0]
    if kind == "grid":
        layers = grid_layers(rng, dims, tie_columns)
        x = rng.integers(-8, 9, (rows, K)).astype(np.float32)
    elif kind == "select":
        layers = [selection(rng, k, m) for k, m in zip(dims[:-1], dims[1:])]
        x = full_mantissa(rng, (rows, K))
    else:
        layers = [(full_mantissa(rng, (K, dims[1])), None)] + [selection(rng, k, m) for k, m in zip(dims[1:-1], dims[2:])]
        x = np.zeros((rows, K), np.float32)
        r = np.arange(rows)
        x[r, r % K] = np.ldexp(1.0, (r // K + r) % 7 - 3)  # rows r, r + K, ...: every k in every position of a row tile
    return layers, x


def assert_exact(layers, x, head: str = "", grid: bool = False):
    """the case has ONE right f32 answer whatever the summation order: the float64 reference IS an f32 value, element for element (and on a
    grid every partial sum is an integer below 2^24); returns the reference as f32"""
    ref = forward64(layers, x, None, head)
    with np.errstate(over="ignore"):
        as32 = ref["out"].astype(np.float32)
        assert np.array_equal(as32.astype(np.float64), ref["out"])
        for z in ref["pre"]:
            assert np.array_equal(z.astype(np.float32).astype(np.float64), z)
    if grid:
        assert all(m.max() < 2 ** 24 for m in ref["mag"]), [m.max() for m in ref["mag"]]
    return as32


# ---- which kernel serves a layer --------------------------------------------------------------------------------------------------

def family(rows: int, K: int, M: int, sm: int = 0, colmajor: bool = False, aligned: bool = True) -> str:
    """dense.hip: dense_kernel_family at its default switches, restated (sm: 0 none, 1 Softmax, 2 LogSoftmax, 3 ArgMax).  The plan names
    the family of a long aligned row-major scan (rows = 2^20), which the GPU tests compare with this function; a short, unaligned or
    column-major call follows the same rule with its own arguments."""
    g16 = 1 <= M <= 16 and 8 <= K <= 128 and K not in (64, 128) and (K > 32 or M >= 3)
    skinny = 1 <= M <= 16 and 1 <= K <= 32
    if colmajor:
        return "dense_narrow16g_kernel" if K >= 8 and (K > 32 or M >= 3) else "dense_skinny_kernel"
    if g16:
        return "dense_narrow16g_kernel"
    if skinny:
        return "dense_skinny_kernel"
    if M <= 16 and K in (64, 128, 256) and rows >= 4096 and aligned:
        return "dense_narrow16s_kernel"
    if M <= 16 and K % 16 == 0 and K <= 1024 and aligned:
        return "dense_narrow16_kernel"
    if 1 <= M <= 64 and K > 128:
        return "dense_narrow16w_kernel"
    if sm == 3:
        return ""
    if M <= 32 and K % 8 == 0 and K <= 512 and aligned:
        return "dense_narrow_kernel"
    return "dense_kernel"


def dense_kernel_mt(rows: int, M: int, sm: int = 0) -> int:
    """dense.hip: dense(): the output tiles per workgroup of dense_kernel<MT> -- as many as the layer has, halved while the grid stays under
    512 workgroups (128 rows each)"""
    row_blocks = (rows + 127) // 128
    mt = 1 if M <= 32 else 2 if M <= 64 else 4 if M <= 128 else 8
    while sm == 0 and mt > 1 and row_blocks * ((M + 32 * mt - 1) // (32 * mt)) < 512:
        mt >>= 1
    return mt


# ---- the cases --------------------------------------------------------------------------------------------------------------------
# (what serves them, dims).  "what" is a dense.hip family (exec "normal" / "dense_softmax" / "dense_argmax" and the plan's dense_kernels), or
# the exec kind of the fused step that takes the layer away from dense.hip: the load-time chain kernel, the fused MLP, the tiled kernel.

ROWS = (1, 31, 33, 257)
BIG = 4096 + 33  # dense_narrow16s_kernel takes rows >= 4096, mlp3_tile16 rows <= 4096

SKINNY = [(k, m) for k in (1, 3, 31, 32) for m in (1, 2, 3, 4, 5, 8, 9, 16) if k < 8 or m < 3]  # MMAX 1 / 2 / 4 / 8 / 16 all among them
G16 = [(k, m) for k in (8, 13, 33, 63, 65, 127) for m in (3, 16)] + [(33, 1), (127, 1)]
N16 = [(k, m) for k in (16, 48, 1024) for m in (1, 7, 16)]
N16S = [(k, m) for k in (64, 128, 256) for m in (1, 10, 16)]  # dense_narrow16_kernel below 4096 rows, dense_narrow16s_kernel from there
W16 = [(k, m) for k in (129, 1025, 2049) for m in (1, 17, 33, 64)]  # 2049: above the BIGK window (weights in the LDS 1024 columns at a time)
NARROW = [(k, m) for k in (8, 24, 512) for m in (17, 32)]
GENERIC = [(5, 17), (130, 33), (36, 65), (20, 129), (12, 300)]
CHAINS = [(9, 20, 4), (30, 100, 2), (4, 10, 3), (17, 40), (5, 8, 8, 1)]
MLP3 = [(128, 256, 64, 1)]


def served_by(dims) -> str:
    """what serves a model of these dims on a GPU (schedule.cpp: fuse_tabular, then dense_kernel_family for a long aligned scan)"""
    if len(dims) == 4 and dims in MLP3:
        return "mlp3_fused"
    if len(dims) > 2:
        return "chain_fused"
    k, m = dims
    if m > 32 and not (k > 128 and m <= 64 and k % 4 != 0):
        # the 32x32 tiled kernel, behind a PadCols where K % 4 != 0 -- which the chain kernel absorbs up to 128 columns and outputs
        return "dense_tiled" if k % 4 == 0 or k > 128 or m > 128 else "chain_fused"
    if 16 < m <= 32 and k % 8 != 0 and k <= 128:  # no aligned kernel reads such rows: a one-layer chain
        return "chain_fused"
    return family(1 << 20, k, m)


# The rows of the issue's table by the kernel they were written for.  Where dense_kernel_family sends a shape elsewhere the shape stays and
# the family that really serves it is the one asserted:
#   dense_narrow16_kernel   K = 16 and 48 belong to dense_narrow16g_kernel (8 <= K <= 128), (16, 1) to dense_skinny_kernel
#   dense_narrow_kernel     K = 512 belongs to dense_narrow16w_kernel (K > 128, M <= 64)
#   dense_kernel<MT>        (5, 17) is a one-layer chain, (130, 33) dense_narrow16w_kernel, the three wide ones the tiled kernel: behind
#                           an aligned pointer no plan reaches dense_kernel for these shapes.  It runs (MT = 1) where K = 64 / 128 rows
#                           start off a 16-byte boundary -- the unaligned calls of N16S below.
TABLE = ([("dense_skinny_kernel", d) for d in SKINNY] + [("dense_narrow16g_kernel", d) for d in G16] + [("dense_narrow16_kernel", d) for d in N16] +
         [("dense_narrow16s_kernel", d) for d in N16S] + [("dense_narrow16w_kernel", d) for d in W16] + [("dense_narrow_kernel", d) for d in NARROW] +
         [("dense_kernel", d) for d in GENERIC] + [("chain_fused", d) for d in CHAINS] + [("mlp3_fused", d) for d in MLP3])
ELSEWHERE = {(16, 1): "dense_skinny_kernel", (16, 7): "dense_narrow16g_kernel", (16, 16): "dense_narrow16g_kernel", (48, 1): "dense_narrow16g_kernel",
             (48, 7): "dense_narrow16g_kernel", (48, 16): "dense_narrow16g_kernel", (512, 17): "dense_narrow16w_kernel", (512, 32): "dense_narrow16w_kernel",
             (5, 17): "chain_fused", (130, 33): "dense_narrow16w_kernel", (36, 65): "dense_tiled", (20, 129): "dense_tiled", (12, 300): "dense_tiled"}
KINDS = ("grid", "select", "onehot")


def expected(row: str, dims) -> str:
    return ELSEWHERE.get(tuple(dims), row)


def case_id(c):
    return c[0].replace("dense_", "").replace("_kernel", "") + "-" + "x".join(map(str, c[1]))


def big_rows(dims) -> bool:
    """the shapes whose kernel changes at a row threshold"""
    return tuple(dims) in N16S or tuple(dims) in MLP3


# one (K, M) per family with a fused ArgMax / Softmax epilogue, and where it runs: aligned rows, rows >= 4096, a column-major chunk
EPILOGUES = [("dense_skinny_kernel", (3, 5), "rows"), ("dense_narrow16g_kernel", (33, 16), "rows"), ("dense_narrow16_kernel", (1024, 7), "rows"),
             ("dense_narrow16_kernel", (128, 10), "rows"), ("dense_narrow16s_kernel", (128, 10), "big"), ("dense_narrow16w_kernel", (129, 33), "rows"),
             ("dense_narrow16w_kernel", (2049, 17), "rows"), ("dense_skinny_kernel", (3, 5), "columns"), ("dense_narrow16g_kernel", (33, 16), "columns")]

# section 3: dims, activations (None: Relu between the layers), final Softmax
GENERIC_DATA = [((3, 5), None, True), ((33, 16), None, False), ((1024, 7), None, True), ((128, 10), None, True), ((129, 33), None, False),
                ((2049, 17), None, True), ((24, 32), None, False), ((5, 17), None, False), ((36, 65), None, False),
                ((9, 20, 4), None, True), ((30, 100, 2), None, True), ((4, 10, 3), None, True), ((17, 40), None, False), ((5, 8, 8, 1), None, False),
                ((128, 256, 64, 1), None, False), ((130, 33, 70, 9), ["Sigmoid", "Tanh", "LeakyRelu"], False)]


def generic_inputs(K, rows: int = 257):
    """synth.table's uniform [-1, 1) values, and columns of 1000 +- 1: sums that cancel"""
    from infera_amd import synth

    off = (1000 + np.random.default_rng(K).uniform(-1, 1, (rows, K))).astype(np.float32)
    return {"uniform": synth.table(21, 0, rows, K), "offset": off}


def rms(a):
    return float(np.sqrt(np.mean(np.square(np.asarray(a, np.float64)))))
