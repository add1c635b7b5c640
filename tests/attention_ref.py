"""float64 restatements of the Transformer kernels (hip/attention.hip, hip/layernorm.hip: Attention, LayerNorm, MeanTime), float32 numpy
restatements of their documented arithmetic, the inputs that take them to their edges, and ONE verdict rule (eltwise_ref.verdict_ref: the
project bar 1e-4 |ref| + 1e-6, NaN and +-inf matched exactly).  numpy only: tests/test_attention_ref.py checks this module without a GPU,
tests/test_attention_range_gpu.py compares the kernels with it on one.

The score of (query i, key j) is an f32 value twice in the operator's definition: fl32(scale . q_i . k_j), and fl32(that + mask[i, j]).
attention() computes the product and the sum in float64 and rounds to float32 at those two places; softmax and P V follow in float64.
The rounding is what makes a finite "minus infinity" well defined: fl32(s - 1e9) is a multiple of 64 (|s| < 32 vanishes in it), and
fl32(s + finfo.min) is finfo.min, so a query whose keys are all masked that way has equal scores and uniform weights, as the f32 operator
gives it.  A true -inf is a weight of exactly 0.

Exact scores.  The builders below draw Q and K from an integer grid (entries n . step, |n| <= G, step a power of two) and take a power of two
as the scale, so scale . q . k = scale . step^2 . (an integer of magnitude <= dh G^2 < 2^24) is a float32 whatever the order of the sum.
The first rounding then never happens, in the kernel or in any restatement, and a score range of thousands is a fair case: what is left
to differ is expf and the accumulations.  exact_case() asserts float32(s) == s on the float64 scores.

Non-finite inputs: NONFINITE below, derived from the f32 definition (0 . NaN = NaN, inf - inf = NaN); attention() evaluates that
definition literally (numpy's IEEE arithmetic), so it is the table's check (tests/test_attention_ref.py)."""
from __future__ import annotations

import math

import numpy as np

from infera_amd import onnx_writer as W
from tests import eltwise_ref as E

RTOL, ATOL = E.RTOL, E.ATOL
f32 = np.float32
FMIN = float(np.finfo(np.float32).min)


def verdict(got, ref) -> float:
    """the worst |got - ref| / (1e-4 |ref| + 1e-6) over the elements, by the rule of eltwise_ref.verdict_ref: a NaN or an infinity of the
    reference (rounded to float32) has to be matched and counts as 0; a non-finite result where the reference is finite, or an unmatched
    NaN / infinity, is inf.  <= 1 passes, and only then does verdict_ref pass every element."""
    got = np.ascontiguousarray(got, np.float32)
    ref = np.asarray(ref, np.float64).reshape(got.shape)
    ok, ratio = E.verdict_ref(got, ref)
    with np.errstate(all="ignore"):
        both = np.isfinite(got) & np.isfinite(ref.astype(np.float32))
        raw = np.abs(got.astype(np.float64) - ref) / (RTOL * np.abs(ref) + ATOL)
    worst = float(np.max(np.where(ok, ratio, np.where(both, raw, np.inf))))
    assert (worst <= 1.0) == bool(ok.all())
    return worst


# ---- attention ------------------------------------------------------------------------------------------------------------------------

def heads_of(a, h):
    """[N, T, E] -> [N, h, T, dh]"""
    N, T, Em = a.shape
    return a.reshape(N, T, h, Em // h).transpose(0, 2, 1, 3)


def mask_tt(mask, T):
    """the mask as the [T, T] table ONNX broadcasting against [N, h, T, T] makes of it (float64); None -> None"""
    if mask is None:
        return None
    mk = np.asarray(mask, np.float32)
    lead = mk.shape[:-2] if mk.ndim > 2 else ()
    assert all(d == 1 for d in lead), mk.shape
    mk = mk.reshape(mk.shape[-2:] if mk.ndim >= 2 else mk.shape)
    return np.broadcast_to(mk, (T, T)).astype(np.float64)


def scores64(q, k, h, scale):
    """scale . q . k per (row, head, query, key) in float64, unrounded"""
    q, k = (heads_of(np.asarray(a, np.float64), h) for a in (q, k))
    with np.errstate(all="ignore"):
        return np.einsum("nhqd,nhkd->nhqk", q, k) * float(scale)


def rounded_scores(q, k, h, scale, mask):
    """fl32(fl32(scale . q . k) + mask) as float64"""
    T = np.shape(q)[1]
    with np.errstate(all="ignore"):
        s = scores64(q, k, h, scale).astype(np.float32).astype(np.float64)
        if mask is not None:
            s = (s + mask_tt(mask, T)).astype(np.float32).astype(np.float64)
    return s


def attention(q, k, v, h: int, scale: float, mask=None) -> np.ndarray:
    """softmax(fl32(fl32(scale . Q K^T) + mask)) V per head over q, k, v [N, T, E] -> [N, T, E], float64.  IEEE all the way: a NaN score
    makes its query NaN (the maximum propagates it), a score of -inf is a weight of exactly 0, 0 . NaN = NaN in P V."""
    N, T, Em = np.shape(q)
    s = rounded_scores(q, k, h, scale, mask)
    with np.errstate(all="ignore"):
        s = s - np.max(s, axis=-1, keepdims=True)  # (np.max propagates NaN; -inf - -inf and inf - inf are NaN)
        p = np.exp(s)
        p = p / p.sum(axis=-1, keepdims=True)
        out = np.einsum("nhqk,nhkd->nhqd", p, heads_of(np.asarray(v, np.float64), h))  # (plain loops: no zero is skipped)
    return out.transpose(0, 2, 1, 3).reshape(N, T, Em)


def attention32(q, k, v, h: int, scale: float, mask=None, tile: int = 16) -> np.ndarray:
    """The same operator in float32 numpy with the kernel's recurrence: keys in tiles of `tile`, a running maximum m and sum l per query,
    o and l rescaled by expf(m_old - m_new) per tile, a -inf score excluded before the maximum.  Not the kernel's bits (its products run on
    the MFMA in another order); it says what float32 itself costs on a case."""
    N, T, Em = np.shape(q)
    qh, kh, vh = (heads_of(np.asarray(a, np.float32), h) for a in (q, k, v))
    mk = None if mask is None else mask_tt(mask, T).astype(np.float32)
    m = np.full((N, h, T, 1), -np.inf, np.float32)
    l = np.zeros((N, h, T, 1), np.float32)
    o = np.zeros((N, h, T, Em // h), np.float32)
    with np.errstate(all="ignore"):
        for k0 in range(0, T, tile):
            s = np.matmul(qh, kh[:, :, k0:k0 + tile].transpose(0, 1, 3, 2)) * f32(scale)
            if mk is not None:
                s = s + mk[:, k0:k0 + tile]
            m_new = np.maximum(m, np.max(s, axis=-1, keepdims=True))
            corr = np.where(np.isneginf(m_new), f32(1), np.exp(m - m_new)).astype(np.float32)
            p = np.where(np.isneginf(s), f32(0), np.exp(s - m_new)).astype(np.float32)
            l = l * corr + p.sum(axis=-1, keepdims=True, dtype=np.float32)
            o = o * corr + np.matmul(p, vh[:, :, k0:k0 + tile])
            m = m_new
        out = o / l
    return out.transpose(0, 2, 1, 3).reshape(N, T, Em)


# What one non-finite element does, from the f32 definition s = scale . (q . k) + mask, p = softmax(s), out = p V with every product
# formed (0 . NaN = NaN, inf - inf = NaN).  Key: (tensor, value); i, j, d: the query / key step and the head column it sits at.
#   Q  NaN        every score of query i is NaN                                   -> query i of that head NaN, nothing else
#   Q  +-inf      the scores of query i are +-inf or NaN (0 . inf); a +inf or NaN score makes the maximum +inf / NaN and
#                 inf - inf = NaN, and scores that are all -inf give -inf - -inf   -> query i of that head NaN, nothing else
#   K  NaN        the score of every query against key j is NaN (NaN + mask too)  -> every query of that (row, head) NaN
#   K  +-inf      the score of query i against key j is q[i, d] . (+-inf): NaN where q[i, d] = 0, +inf where the signs agree -- both
#                 make query i NaN, whatever the mask adds to it but -inf to +inf, which is NaN as well -- and -inf where they
#                 differ: key j then has weight exactly 0 for query i, as under a -inf mask entry, and query i stays finite unless
#                 j was its only key.  Every query of the (row, head) is NaN exactly where no q[i, d] has the opposite sign.
#   V  NaN        p[i, j] . NaN = NaN for every i, p[i, j] = 0 included          -> column d of every query of that head NaN
#   V  +-inf      p[i, j] . inf = +-inf where p[i, j] > 0, NaN where it is 0       -> column d: +-inf where the weight is positive,
#                                                                                    NaN where it is exactly 0 (masked by -inf)
# Other heads and other rows never meet the element: bit-identical to the clean run.
NONFINITE = {
    ("Q", "nan"): "query", ("Q", "+inf"): "query", ("Q", "-inf"): "query",
    ("K", "nan"): "head", ("K", "+inf"): "head-by-sign", ("K", "-inf"): "head-by-sign",
    ("V", "nan"): "column", ("V", "+inf"): "column-by-weight", ("V", "-inf"): "column-by-weight",
}
VALUES = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf}


def nonfinite_expectation(effect, value, qh, mask, i, j, d):
    """NONFINITE as arrays for one head: (nan [T, dh] bool, inf [T, dh] float: 0 where finite or NaN, else the infinity).  qh: that head's
    clean Q [T, dh]; mask: None or what mask_tt() takes; `value` the planted number; i / j: the step, d: the column."""
    T, dh = qh.shape
    nan, inf = np.zeros((T, dh), bool), np.zeros((T, dh))
    mk = np.zeros((T, T)) if mask is None else mask_tt(mask, T)
    if effect == "query":
        nan[i] = True
    elif effect == "head":
        nan[:] = True
    elif effect == "head-by-sign":
        with np.errstate(all="ignore"):
            prod = qh[:, d].astype(np.float64) * value + mk[:, j]  # NaN, +inf or -inf
        only_key = np.isneginf(np.delete(mk, j, axis=1)).all(axis=1)
        nan[~np.isneginf(prod) | only_key] = True
    elif effect == "column":
        nan[:, d] = True
    else:
        assert effect == "column-by-weight", effect
        zero = np.isneginf(mk[:, j])
        nan[zero, d] = True
        inf[~zero, d] = value
    return nan, inf


# ---- exact-score inputs ---------------------------------------------------------------------------------------------------------------

# name -> (step, G): Q and K entries are n . step with integer |n| <= G
RANGES = {"unit": (0.25, 16), "wide": (1.0, 16), "huge": (1.0, 64)}
ORDERS = ("random", "ascending", "descending")


def exact_case(T: int, dh: int, h: int, rows: int, rng_name: str, scale: float, order="random", seed: int = 0):
    """(q, k, v) [rows, T, h dh] float32 with exact scores (module docstring): Q and K entries are n . step, n an integer in [-G, G]
    (RANGES[rng_name]); `scale` is a power of two.  Then scale . q . k = scale . step^2 . sum(n n'), an integer of magnitude <= dh G^2
    (2^18 at dh = 64, G = 64) times a power of two: a float32, asserted here on the float64 scores.  V is uniform(-1, 1).
    order: "random": n uniform.
           "ascending": per head a sign vector u; q = |n| u with n in [G / 2, G], k_j = floor(G j / (T - 1)) u + one of {-1, 0, 1} in one
               column (clipped to the grid): a step of the amplitude moves q . k_j by sum|n| >= dh G / 2, the noise by at most G: asserted -- for
               every query the maximum over each 16-key sub-tile exceeds the maximum over all keys before it.
           "descending": the same keys in reverse.
           an integer p: random keys of |n| <= G / 4, key p = G u and q = |n| u (n in [G / 2, G]): key p's score exceeds every other by construction."""
    step, G = RANGES[rng_name]
    assert math.frexp(scale)[0] == 0.5 and math.frexp(step)[0] == 0.5 and dh * G * G < 2 ** 24, (scale, step, dh, G)
    rng = np.random.default_rng([seed, T, dh, h, G, 0 if isinstance(order, str) else 1 + order])
    shape = (rows, T, h, dh)
    if order == "random":
        qn, kn = rng.integers(-G, G + 1, shape), rng.integers(-G, G + 1, shape)
    else:
        u = rng.choice([-1, 1], (1, 1, h, dh))
        qn = rng.integers(G // 2, G + 1, shape) * u
        if isinstance(order, str):
            amp = (G * np.arange(T) // max(T - 1, 1)).reshape(1, T, 1, 1)
            noise = rng.integers(-1, 2, shape) * (rng.integers(0, dh, (rows, T, h, 1)) == np.arange(dh))
            kn = np.clip(amp * u + noise, -G, G)
            if order == "descending":
                kn = kn[:, ::-1]
        else:
            kn = rng.integers(-(G // 4), G // 4 + 1, shape)
            kn[:, order] = G * u[:, 0]
    q, k = (np.ascontiguousarray((a * step).reshape(rows, T, h * dh), np.float32) for a in (qn, kn))
    v = rng.uniform(-1, 1, (rows, T, h * dh)).astype(np.float32)
    s = scores64(q, k, h, scale)
    assert np.array_equal(s.astype(np.float32).astype(np.float64), s), "scores are not exact in float32"
    if order in ("ascending", "descending"):
        sa = s if order == "ascending" else s[..., ::-1]
        sub = np.stack([sa[..., c:c + 16].max(-1) for c in range(0, T, 16)], -1)
        assert (np.diff(sub, axis=-1) > 0).all(), "the running maximum does not rise in every sub-tile"
    elif order != "random":
        assert (s[..., order:order + 1] > np.delete(s, order, axis=-1)).all(), "key %d does not dominate" % order
    return q, k, v


def unit_case(T: int, E_: int, rows: int, seed: int = 0):
    """(q, k, v) uniform(-1, 1): layout and geometry cases, where the scores need not be exact"""
    rng = np.random.default_rng([seed, T, E_])
    return tuple(rng.uniform(-1, 1, (rows, T, E_)).astype(np.float32) for _ in range(3))


# ---- masks ----------------------------------------------------------------------------------------------------------------------------

def banded(T, w):
    """query i sees keys i - w .. i"""
    i, j = np.arange(T)[:, None], np.arange(T)[None, :]
    return np.where((j <= i) & (j >= i - w), 0.0, -np.inf).astype(np.float32)


def left_padding(T):
    """keys 0..16 masked for queries >= 17 (an all -inf leading 16-key sub-tile), keys 0..31 for queries >= 32 (an all -inf 32-key tile)"""
    mk = np.zeros((T, T), np.float32)
    mk[17:32, :17] = -np.inf
    mk[32:, :32] = -np.inf
    return mk


def causal(T, fill=-np.inf):
    return np.triu(np.full((T, T), fill, dtype=np.float32), 1)


def full_row(T, fill, row=None):
    """causal, but query `row` (default T // 2) is `fill` at EVERY key: equal rounded scores only where fill absorbs them"""
    mk = causal(T)
    mk[T // 2 if row is None else row, :] = fill
    return mk


def alibi(T):
    i, j = np.arange(T)[:, None], np.arange(T)[None, :]
    return (-np.abs(i - j) / 16.0).astype(np.float32)


def key_mask(T, shape):
    """every third key from 1 masked, as [1, T], [T] or [1, 1, 1, T]"""
    mk = np.zeros(T, np.float32)
    mk[1::3] = -np.inf
    return mk.reshape(shape)


def query_bias(T):
    """[T, 1]: one number per query, finite (softmax is invariant to it up to the rounding of the sum)"""
    return (np.arange(T, dtype=np.float32).reshape(T, 1) % 7 - 3) * f32(0.5)


# name -> T -> mask: the families of the -inf branch, the finite "minus infinities", finite biases and the broadcast shapes
MASKS = {
    "band3": lambda T: banded(T, 3), "band20": lambda T: banded(T, 20), "leftpad": left_padding,
    "causal-1e9": lambda T: causal(T, -1e9), "causal-1e4": lambda T: causal(T, -10000.0), "causal-fmin": lambda T: causal(T, FMIN),
    "row-1e9": lambda T: full_row(T, -1e9), "row-fmin": lambda T: full_row(T, FMIN), "alibi": alibi,
    "key[1,T]": lambda T: key_mask(T, (1, T)), "key[T]": lambda T: key_mask(T, (T,)), "key[1,1,1,T]": lambda T: key_mask(T, (1, 1, 1, T)),
    "query[T,1]": query_bias,
}
INF_KINDS = ("band3", "band20", "leftpad")  # late queries meet an all -inf leading sub-tile and a whole -inf 32-key tile (bands: T >= 65)


def attention_graph(T, dh, h, form="packed", mask=None, scale_value=None, mask_left=False):
    """attention alone; a given scale_value is written as Mul of the scores by that f32, so the folded scale is the number itself"""
    kw = dict(mask=mask, mask_left=mask_left)
    if scale_value is not None:
        kw.update(scale="scores_mul", scale_value=scale_value)
    return W.attention_only(T, dh * h, h, form=form, **kw)


def pack(q, k, v, form="packed"):
    """the call's table: "packed" [rows, T 3E] (q | k | v per step), "three" [rows, 3 T E] (Q, K, V one after the other)"""
    rows = q.shape[0]
    if form == "packed":
        return np.ascontiguousarray(np.concatenate([q, k, v], axis=-1).reshape(rows, -1))
    return np.ascontiguousarray(np.concatenate([a.reshape(rows, -1) for a in (q, k, v)], axis=1))


# ---- LayerNorm and MeanTime -----------------------------------------------------------------------------------------------------------

def layernorm(x, g, b, eps) -> np.ndarray:
    """(x - mean) / sqrt(var + eps) . gamma + beta over the last axis in float64; eps as the f32 the kernel holds"""
    x = np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        d = x - x.mean(axis=-1, keepdims=True)
        y = d / np.sqrt((d * d).mean(axis=-1, keepdims=True) + np.float64(np.float32(eps))) * np.asarray(g, np.float64)
        return y if b is None else y + np.asarray(b, np.float64)


def layernorm32(x, g, b, eps) -> np.ndarray:
    """the documented formula in float32 numpy: mean = sum / E; d = x - mean; d -= sum(d) / E; var = sum(d^2) / E;
    y = d / sqrtf(var + eps) . gamma + beta.  numpy's sums are pairwise, the kernel's a butterfly: the same formula, not the same bits."""
    x = np.asarray(x, np.float32)
    n = f32(x.shape[-1])
    with np.errstate(all="ignore"):
        d = x - x.sum(axis=-1, keepdims=True, dtype=np.float32) / n
        d = d - d.sum(axis=-1, keepdims=True, dtype=np.float32) / n
        var = (d * d).sum(axis=-1, keepdims=True, dtype=np.float32) / n
        y = d / np.sqrt(var + f32(eps)) * np.asarray(g, np.float32)
        return y if b is None else y + np.asarray(b, np.float32)


def mean_time(x) -> np.ndarray:
    """[N, T, E] -> [N, E] in float64"""
    with np.errstate(all="ignore"):
        return np.asarray(x, np.float64).mean(axis=1)


LN_FAMILY_E = (3, 33, 768, 4095)
LN_FAMILIES = ("scale1e-18", "scale1e-6", "scale1e6", "scale1e15", "const0", "const0.1", "const1000", "const1e6", "outlier1e4", "offset1e5",
               "gamma0neg")
LN_EPS = (1e-12, 1e-5, 1e-3)


def ln_inputs(family: str, E_: int, rows: int = 37, seed: int = 0):
    """(x [rows, E] f32, gamma, beta) of one input family"""
    rng = np.random.default_rng([seed, E_, LN_FAMILIES.index(family)])
    u = rng.uniform(-1, 1, (rows, E_)).astype(np.float32)
    g, b = rng.normal(1, 0.2, E_).astype(np.float32), rng.normal(0, 0.2, E_).astype(np.float32)
    if family.startswith("scale"):
        u = u * f32(float(family[5:]))
    elif family.startswith("const"):
        u[:] = f32(float(family[5:]))
    elif family == "outlier1e4":
        u[np.arange(rows), (5 * np.arange(rows)) % E_] = 1e4
    elif family == "offset1e5":
        u = u + f32(1e5)
    else:
        assert family == "gamma0neg", family
        g[0::3], g[1::3] = 0.0, -g[1::3]
    return np.ascontiguousarray(u, np.float32), g, b


def layernorm_graph(E_: int, eps: float, g, b=None, T: int = 0) -> bytes:
    """LayerNormalization(axis -1) on [N, E] (T = 0) or on [N, T, E] behind a Reshape; B optional"""
    inits = [W.tensor("g", np.asarray(g, np.float32))] + ([] if b is None else [W.tensor("b", np.asarray(b, np.float32))])
    nodes = []
    if T:
        inits.append(W.tensor("s", np.asarray([-1, T, E_], np.int64)))
        nodes.append(W.node("Reshape", ["X", "s"], ["x3"]))
    nodes.append(W.node("LayerNormalization", ["x3" if T else "X", "g"] + ([] if b is None else ["b"]), ["out"],
                        [W.attr_i("axis", -1), W.attr_f("epsilon", eps)], name="ln"))
    return W.model("ln", nodes, inits, [W.value_info("X", ["N", max(T, 1) * E_])], [W.value_info("out", ["N", T, E_] if T else ["N", E_])], opset=20)


def mean_time_graph(T: int, E_: int, keepdims: int) -> bytes:
    nodes = [W.node("Reshape", ["X", "s"], ["x3"]), W.node("ReduceMean", ["x3", "ax"], ["out"], [W.attr_i("keepdims", keepdims)])]
    inits = [W.tensor("s", np.asarray([-1, T, E_], np.int64)), W.tensor("ax", np.asarray([1], np.int64))]
    return W.model("mt", nodes, inits, [W.value_info("X", ["N", T * E_])], [W.value_info("out", ["N", 1, E_] if keepdims else ["N", E_])], opset=20)


# ---- the case lists of tests/test_attention_range_gpu.py (tests/test_attention_ref.py walks the same lists without a GPU) ------------

# (T, dh, h, scale): scale is written as Mul of the scores by that power of two (dh = 5: an explicit 0.5, not 1 / sqrt(dh))
# T = 33, 65, 129 all end in a sub-tile of ONE key with an even index, whose rescale wipes what the ascending order left before it;
# T = 64 ends in a full second sub-tile, so an error made there is still in the result.
SCORE_SHAPES = [(T, dh, h, sc) for dh, h, sc in ((16, 2, 0.25), (64, 2, 0.125), (5, 3, 0.5)) for T in (33, 65, 129)] + [(64, 16, 2, 0.25)]


def score_orders(T):
    """random, ascending, descending, and the one dominant key at 0, 15, 16, 31, 32 and T - 1"""
    return list(ORDERS) + [0, 15, 16, 31, 32, T - 1]


MASK_T = (33, 65, 100)
MASK_KINDS = tuple(MASKS) + ("band3-left",)  # the last: the mask as the left operand of the Add
MASK_RANGES = ("unit", "wide")
MASK_SHAPE = (16, 2, 0.25)  # dh, h, scale
ROWS = 7

# torch float32 layer_norm on the CPU against layernorm() over LN_FAMILY_E x LN_EPS (tests/test_attention_ref.py asserts the split):
# every family stays within 0.18 of the bar but the common offset of 1e5, where torch's variance misses it 1e3 - 2e4 times over.
LN_ASSERTED = tuple(f for f in LN_FAMILIES if f != "offset1e5")
LN_BOUNDARY_E = (31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 4095, 4096)
