"""The ONNX LSTM / GRU / RNN definition in numpy, the inputs that take rnn_kernel<OP> (hip/rnn.hip) to its shape
and value edges, and ONE verdict rule (eltwise_ref.verdict_ref: the project bar 1e-4 |ref| + 1e-6, NaN and +-inf matched exactly).  numpy only:
tests/test_recurrent_ref.py checks this module without a GPU, tests/test_recurrent_range_gpu.py compares the kernel with it on one.

recurrent(spec, x) is the definition in float64; recurrent(spec, x, np.float32) is the same statement with every product, sum and activation
in float32 -- not the kernel's bits (its sums are k-ordered fma chains on the MFMA), but what float32 itself costs on a case: a case is a fair
one for the bar only where that restatement stays within a quarter of it (the rule of tests/test_recurrent_gpu.py, case by case).

Exact cases.  grid_relu_rnn() builds a ReLU RNN whose weights, biases, initial state and inputs are small integers.  Every pre-activation is
then a sum of integers; where the sum of the TERM MAGNITUDES stays below 2^24 every partial sum in every order is an integer below 2^24, so
float32 computes the float64 result exactly and the served Y can be compared bit for bit.  assert_exact() establishes that bound from the
float64 reference alone.  R has one non-zero per row, at column (5 i + 3) mod H: the state does not grow geometrically (one term per step),
each unit reads another unit's previous value, and the pattern is not symmetric -- a transposed or shifted R, a swapped k-group of W, a
stale h copy or a padded unit that is not 0 changes integers, which no tolerance hides.

Non-finite inputs: numpy's IEEE arithmetic evaluates the definition literally (inf - inf and 0 . inf are NaN; sigmoid(+-inf) is 1 / 0 and
tanh(+-inf) is +-1, so an infinite reading saturates the gates of its step and the row stays finite where no such NaN arises)."""
from __future__ import annotations

import copy
import functools

import numpy as np

from infera_amd import onnx_writer as W
from tests import eltwise_ref as E

RTOL, ATOL = E.RTOL, E.ATOL
GATES = {"LSTM": ("i", "o", "f", "c"), "GRU": ("z", "r", "h"), "RNN": ("h",)}  # ONNX order


def recurrent(spec, x, dtype=np.float64, probe=None):
    """x [N, T, F] -> (Y [N, T, D*H] of the last layer, Y_h [N, D*H], Y_c [N, D*H] or None), all in `dtype`: float64 is the definition,
    float32 the restatement that rounds every product, sum and activation to float32.  probe(x_t, h, W, R, Wb, Rb), if given, sees the
    operands of every step of every layer and direction."""
    op, H, D = spec["op"], spec["H"], spec["D"]
    G = len(GATES[op])
    one = dtype(1)
    as_t = lambda a: np.asarray(a).astype(dtype)  # noqa: E731
    sig = lambda v: one / (one + np.exp(-v))  # noqa: E731
    g = lambda a, k: a[..., k * H:(k + 1) * H]  # noqa: E731
    dot = np.matmul if dtype == np.float64 else _dot32
    x = as_t(x)
    N, T, _ = x.shape
    with np.errstate(all="ignore"):
        for L in spec["layers"]:
            ys, hs, cs = [], [], []
            for d in range(D):
                Wm, Rm = as_t(L["W"][d]), as_t(L["R"][d])
                B = as_t(L["B"][d]) if L["B"] is not None else np.zeros(2 * G * H, dtype)
                Wb, Rb = B[:G * H], B[G * H:]
                h = np.tile(as_t(L["h0"][d]), (N, 1)) if L.get("h0") is not None else np.zeros((N, H), dtype)
                c = np.tile(as_t(L["c0"][d]), (N, 1)) if L.get("c0") is not None else np.zeros((N, H), dtype)
                rev = spec["direction"] == "reverse" or d == 1
                y = np.zeros((N, T, H), dtype)
                for t in (range(T - 1, -1, -1) if rev else range(T)):
                    if probe is not None:
                        probe(x[:, t], h, Wm, Rm, Wb, Rb)
                    xw, hr = dot(x[:, t], Wm.T) + Wb, dot(h, Rm.T) + Rb
                    if op == "LSTM":
                        i, o, f, cc = sig(g(xw, 0) + g(hr, 0)), sig(g(xw, 1) + g(hr, 1)), sig(g(xw, 2) + g(hr, 2)), np.tanh(g(xw, 3) + g(hr, 3))
                        c = f * c + i * cc
                        h = o * np.tanh(c)
                    elif op == "GRU":
                        z, r = sig(g(xw, 0) + g(hr, 0)), sig(g(xw, 1) + g(hr, 1))
                        if spec["linear_before_reset"]:
                            hh = np.tanh(g(xw, 2) + r * g(hr, 2))
                        else:
                            hh = np.tanh(g(xw, 2) + dot(r * h, g(Rm.T, 2)) + g(Rb, 2))
                        h = (one - z) * hh + z * h
                    else:
                        v = xw + hr
                        h = np.maximum(v, 0) if spec["activation"] == "Relu" else np.tanh(v)
                    assert h.dtype == dtype and c.dtype == dtype
                    y[:, t] = h
                ys.append(y), hs.append(h), cs.append(c)
            x = np.concatenate(ys, axis=2)
    return x, np.concatenate(hs, axis=1), (np.concatenate(cs, axis=1) if op == "LSTM" else None)


def _dot32(a, b):
    """a [N, K] . b [K, M] in float32 as one chain per output, k ascending, every product and every sum rounded: the same numbers on every
    machine (a BLAS picks its summation order by the CPU it finds)"""
    acc = np.zeros((a.shape[0], b.shape[1]), np.float32)
    for k in range(a.shape[1]):
        acc += a[:, k, None] * b[k]
    return acc


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


def bits(a):
    """the uint32 view of a float32 array (of a float64 one: rounded to float32 first)"""
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the exact grid -----------------------------------------------------------------------------------------------------------------------

def grid_relu_rnn(T, F, H, D=1, layers=1, seed=0, initial=False, direction=None):
    """A ReLU RNN spec of integers (module docstring): W in [-2, 2], R one +-1 per row at column (5 i + 3) mod H, B in [-3, 3], h0 (initial)
    one row in [-4, 4] per layer and direction.  direction: "forward" / "reverse" for D = 1 (default forward), "bidirectional" for D = 2."""
    direction = direction or ("bidirectional" if D == 2 else "forward")
    assert D == (2 if direction == "bidirectional" else 1)
    rng = np.random.default_rng([seed, T, F, H, D, layers])
    f32 = lambda a: np.asarray(a, dtype=np.float32)  # noqa: E731
    ls = []
    for i in range(layers):
        fin = F if i == 0 else D * H
        R = np.zeros((D, H, H))
        R[:, np.arange(H), (5 * np.arange(H) + 3) % H] = rng.choice([-1, 1], (D, H))
        ls.append({"W": f32(rng.integers(-2, 3, (D, H, fin))), "R": f32(R), "B": f32(rng.integers(-3, 4, (D, 2 * H))),
                   "h0": f32(rng.integers(-4, 5, (D, H))) if initial else None, "c0": None})
    return {"op": "RNN", "T": T, "F": F, "H": H, "D": D, "direction": direction, "linear_before_reset": 1, "activation": "Relu", "layers": ls}


def grid_inputs(rows, T, F, seed=0, lim=4):
    """integers in [-lim, lim] as float32 [rows, T, F]"""
    return np.random.default_rng([seed, rows, T, F]).integers(-lim, lim + 1, (rows, T, F)).astype(np.float32)


def assert_exact(spec, x):
    """From the float64 reference alone: every operand of every step, layer and direction is an integer, and every pre-activation's sum of
    term magnitudes sum|w x| + sum|r h| + |Wb| + |Rb| is below 2^24.  Then every partial sum in any order is an integer below 2^24 and
    float32 arithmetic gives the float64 result.  Returns that result (Y, Y_h, None)."""
    assert spec["op"] == "RNN" and spec["activation"] == "Relu", spec["op"]
    worst = [0.0]

    def probe(xt, h, Wm, Rm, Wb, Rb):
        for a in (xt, h, Wm, Rm, Wb, Rb):
            assert np.array_equal(a, np.rint(a)), "not an integer grid"
        worst[0] = max(worst[0], float((np.abs(xt) @ np.abs(Wm).T + np.abs(h) @ np.abs(Rm).T + np.abs(Wb) + np.abs(Rb)).max()))

    out = recurrent(spec, x, np.float64, probe)
    assert worst[0] < 2 ** 24, worst[0]
    return out


def swapped(spec, what):
    """A copy of a grid spec with two columns of every R exchanged (what = "R": the columns units 0 and 1 read, 3 mod H and 8 mod H), or two
    k-groups of the first layer's W (what = "W": the first two groups of 16 features, of 4 below F = 32, single features below F = 8).
    None where there is nothing to exchange (H = 1, F = 1)."""
    s = copy.deepcopy(spec)
    H, F = s["H"], s["F"]
    if what == "R":
        a, b = 3 % H, 8 % H
        if a == b:
            return None
        for L in s["layers"]:
            L["R"][:, :, [a, b]] = L["R"][:, :, [b, a]]
        return s
    k = 16 if F >= 32 else 4 if F >= 8 else 1
    if F < 2 * k:
        return None
    Wm = s["layers"][0]["W"]
    Wm[:, :, :2 * k] = np.concatenate([Wm[:, :, k:2 * k], Wm[:, :, :k]], axis=2)
    return s


# (T, F, H) forward at rows 1, 16, 17 and 33 of one 33-row table: one unit; the smallest shape whose x_t fetch reaches commit()'s tail
# loop (one wave prefetches 128 of the 16 . 9 = 144 elements); a padded second tile; 8 tiles on 8 waves; 9, 13 and 17 tiles dealt
# unevenly over 8 waves (waves that hold no tile q skip MFMAs and LDS writes but meet every barrier); 32 tiles with padding (500);
# dynamic LDS of exactly 64 KB, one k-group above (the opt-in), the opt-in with a single wave, and the caps.
GRID_SHAPES = [(1, 1, 1), (2, 9, 16), (3, 15, 17), (5, 16, 128), (4, 17, 144), (3, 33, 200), (3, 8, 272), (2, 65, 500), (2, 512, 256), (2, 528, 256),
               (2, 1024, 16), (2, 1024, 512)]
GRID_ROWS = (1, 16, 17, 33)
GRID_FORM_SHAPES = [(4, 17, 144), (3, 33, 200)]
# name -> (grid_relu_rnn keywords, [(form, initial) of recurrent_from_spec])
GRID_FORMS = {"reverse": (dict(direction="reverse"), [("batch_first", "const")]),
              "bidirectional2": (dict(D=2, layers=2), [("batch_first", "const")]),
              "initial": (dict(initial=True), [("batch_first", "const"), ("layout1", "expand")])}
# ((T, F, H), grid_relu_rnn keywords, rows) through predict_columns: the column-major staged chunk
GRID_COLUMNS = [((2, 9, 16), {}, 17), ((2, 9, 16), dict(direction="reverse"), 17), ((4, 17, 144), dict(D=2), 17), ((2, 65, 500), {}, 33)]
GRID_LONG = ((4096, 1, 16), 17)  # kRnnMaxT steps: 4096 flips of the h double buffer, forward and reverse


GRID_SEED = 1  # (seed 0 draws W = 0 for the one-unit shape)


def grid_case(shape, kw=None, rows=33, lim=4):
    """(spec, x, (Y, Y_h) float64) of one grid case, exactness asserted"""
    return _grid_case(tuple(shape), tuple(sorted((kw or {}).items())), rows, lim)


@functools.lru_cache(maxsize=None)
def _grid_case(shape, kw, rows, lim):
    T, F, H = shape
    spec = grid_relu_rnn(T, F, H, seed=GRID_SEED, **dict(kw))
    x = grid_inputs(rows, T, F, lim=lim)
    y, yh, _ = assert_exact(spec, x)
    return spec, x, (y, yh)


def all_grid_cases():
    """every (shape, keywords, rows) the GPU suite compares bit for bit"""
    out = [(s, {}, 33) for s in GRID_SHAPES]
    out += [(s, kw, 33) for s in GRID_FORM_SHAPES for kw, _ in GRID_FORMS.values()]
    out += list(GRID_COLUMNS)
    out += [(GRID_LONG[0], dict(direction=d), GRID_LONG[1]) for d in ("forward", "reverse")]
    return out


# ---- the bar cases ------------------------------------------------------------------------------------------------------------------------

OPS = {"LSTM": ("LSTM", {}), "GRU_lbr1": ("GRU", dict(linear_before_reset=1)), "GRU_lbr0": ("GRU", dict(linear_before_reset=0)),
       "RNN_tanh": ("RNN", dict(activation="Tanh"))}


def saturating(spec, gate, sign, by=40.0):
    """A copy of `spec` with sign . 40 added to the input bias Wb of one gate (LSTM i / o / f, GRU z / r) in every layer and direction:
    with inputs of ordinary size that gate is 1 (or 0) to the last bit of float64's sigmoid."""
    names = GATES[spec["op"]]
    assert gate in names[:-1], (spec["op"], gate)
    k, H = names.index(gate), spec["H"]
    s = copy.deepcopy(spec)
    for L in s["layers"]:
        L["B"][:, k * H:(k + 1) * H] += np.float32(sign * by)
    return s


def inputs(rows, T, F, seed=3, scale=1.0):
    return (np.random.default_rng([seed, rows, T, F]).normal(0, 1, (rows, T, F)) * scale).astype(np.float32)


def _case(name, op, T, F, H, rows=33, sat=(), xscale=1.0, tails=(), x="normal", w_scale=1.0, **kw):
    """w_scale multiplies every W, R and B of the seeded spec; the other keywords are recurrent_spec's"""
    return dict(name=name, op=op, T=T, F=F, H=H, rows=rows, sat=tuple(sat), xscale=xscale, tails=tuple(tails), x=x, w_scale=w_scale, kw=kw)


def _tails(op, yes=True):
    return (("y_h", "y_c") if OPS.get(op, (op,))[0] == "LSTM" else ("y_h",)) if yes else ()


TILE_H = (16, 128, 144, 200, 272, 500)  # 1, 8, 9, 13, 17 and 32 tiles
# b. F = 9 (the tail loop of commit() at H = 16), T = 6, 33 rows, U(+-1/sqrt(H)) weights
TILE_CASES = [_case(f"tiles {o} H={H}", o, 6, 9, H, tails=_tails(o, H == 144)) for o in OPS for H in TILE_H]
# w_scale: the two-layer bidirectional tanh RNN gets half the weights, as in tests/test_recurrent_gpu.py (w_scale there): float32 itself uses 0.30
# (H = 144) and 0.36 (H = 272) of the bar at 1.0, 0.06 and 0.18 at 0.5
TILE_CASES += [_case(f"tiles {o} H={H} bidirectional x2 initial", o, 6, 9, H, direction="bidirectional", layers=2, initial=0.5,
                     w_scale=0.5 if o == "RNN_tanh" else 1.0) for o in OPS for H in (144, 272)]
TILE_COLUMNS = [f"tiles GRU_lbr0 H={H}" for H in (144, 272)]

# c. T = 1 and 2 (no flip, one flip of the h double buffer) against the direction; T = 512 at (F = 4, H = 32)
ALL_OPS = list(OPS) + ["RNN_relu"]
TIME_CASES = [_case(f"time {o} T={T} {d}", o, T, 5, 24, tails=("y_h",), direction=d) for o in ALL_OPS for T in (1, 2) for d in ("reverse", "bidirectional")]
# r_scale: float32 stays within a quarter of the bar over 512 steps with R as seeded (0.04 - 0.11 of it: the gates and tanh contract), so
# nothing is contracted but the Relu RNN, whose R has to be a contraction for the state to stay bounded at all (U(+-1/sqrt(32)) . 0.5: a
# spectral norm near 0.6)
LONG_R_SCALE = {"LSTM": 1.0, "GRU_lbr1": 1.0, "GRU_lbr0": 1.0, "RNN_tanh": 1.0, "RNN_relu": 0.5}
LONG_CASES = [_case(f"time {o} T=512 forward", o, 512, 4, 32, r_scale=LONG_R_SCALE[o]) for o in ALL_OPS]
LONG_CASES += [_case("time LSTM T=512 bidirectional", "LSTM", 512, 4, 32, direction="bidirectional", r_scale=LONG_R_SCALE["LSTM"])]

# d. F = 6, H = 40 (padded to 48: three waves), T = 8, inputs x 50; each gate pinned at +-40.
# X50_W_SCALE: with inputs of +-150 a pre-activation is a sum of terms of magnitude ~10 whose float32 roundings (~1e-6) land on outputs that
# cross 0, where the bar is 1e-6: float32 itself uses up to 0.70 of the bar at the seeded weights, up to 0.51 at half of them and at most
# 0.18 at a quarter (the float32 mode of recurrent() against its float64 mode, every case of this family, planted infinities included).  So
# the family runs at a quarter: pre-activations of |x| . |w| ~ 50 . 0.04 per term, saturated on the large readings, and the pinned gate
# (bias +-40, not scaled) saturated on every step.
X50_W_SCALE = 0.25
SAT_GATES = [("LSTM", g) for g in "iof"] + [("GRU_lbr1", g) for g in "zr"] + [("GRU_lbr0", g) for g in "zr"]
SAT_CASES = [_case(f"values {o} {g}{'+' if s > 0 else '-'}40 x50", o, 8, 6, 40, sat=[(g, s)], xscale=50.0, w_scale=X50_W_SCALE, tails=_tails(o)) for o, g in SAT_GATES for s in (1, -1)]
SAT_CASES += [_case("values LSTM f-40 x50 H=144", "LSTM", 8, 6, 144, sat=[("f", -1)], xscale=50.0, w_scale=X50_W_SCALE, tails=_tails("LSTM")),
              _case("values GRU_lbr0 r+40 x50 H=144", "GRU_lbr0", 8, 6, 144, sat=[("r", 1)], xscale=50.0, w_scale=X50_W_SCALE)]
# the identities of the definition, with inputs of ordinary size so that the pinned gate is 1 or 0 to the last bit: z = 1 keeps h0 for
# ever; i = 0 and f = 1 keep c0 for ever
IDENTITY_CASES = [_case("values GRU_lbr1 z+40 keeps h0", "GRU_lbr1", 8, 6, 40, sat=[("z", 1)], initial=0.5),
                  _case("values GRU_lbr0 z+40 keeps h0", "GRU_lbr0", 8, 6, 40, sat=[("z", 1)], initial=0.5),
                  _case("values LSTM i-40 f+40 keeps c0", "LSTM", 8, 6, 40, sat=[("i", -1), ("f", 1)], tails=("y_c",), initial=0.5)]
# i = f = 1 and g held near +1 (the cell gate's input weights made positive, positive inputs): c_t = c_{t-1} + g, c_T ~ T = 512.  The bar is
# relative, so a cell state of hundreds is a fair case as long as float32's own 512 roundings stay within a quarter of it.
GROW_CASE = _case("values LSTM i+40 f+40 c grows T=512", "LSTM", 512, 6, 40, rows=17, sat=[("i", 1), ("f", 1)], tails=("y_c",), x="positive")
INF_CASES = [_case(f"values {o} inf rows x50", o, 8, 6, 40, xscale=50.0, w_scale=X50_W_SCALE) for o in ("LSTM", "GRU_lbr1", "GRU_lbr0", "RNN_tanh")]
INF_AT = ((5, 2, 1, np.inf), (21, 4, 3, -np.inf))  # (row, step, feature, value)
# a ReLU RNN on generic data: R contracted (U(+-1/12) . 0.5 has a spectral norm near 0.6), 9 tiles
RELU_CASE = _case("values RNN_relu H=144", "RNN_relu", 8, 6, 144, r_scale=0.5)

BAR_CASES = {c["name"]: c for c in TILE_CASES + TIME_CASES + LONG_CASES + SAT_CASES + IDENTITY_CASES + [GROW_CASE] + INF_CASES + [RELU_CASE]}


def build(case):
    """(spec, x) of one bar case"""
    op, kw = ("RNN", dict(activation="Relu")) if case["op"] == "RNN_relu" else OPS[case["op"]]
    spec = W.recurrent_spec(op, T=case["T"], F=case["F"], H=case["H"], **kw, **case["kw"])
    if case["w_scale"] != 1.0:
        for L in spec["layers"]:
            for k in ("W", "R", "B"):
                L[k] *= np.float32(case["w_scale"])
    for gate, sign in case["sat"]:
        spec = saturating(spec, gate, sign)
    if case["x"] == "positive":
        H = case["H"]
        for L in spec["layers"]:
            L["W"][:, 3 * H:] = np.abs(L["W"][:, 3 * H:])
        x = np.random.default_rng([7, case["T"]]).uniform(10, 20, (case["rows"], case["T"], case["F"])).astype(np.float32)
    else:
        x = inputs(case["rows"], case["T"], case["F"], scale=case["xscale"])
    return spec, x


def plant_inf(spec, x):
    """x with INF_AT planted; asserts that no weight of the planted feature's column is exactly 0 (0 . inf would be NaN)"""
    x = x.copy()
    for row, t, f, v in INF_AT:
        assert (spec["layers"][0]["W"][:, :, f] != 0).all()
        x[row, t, f] = v
    return x


@functools.lru_cache(maxsize=None)
def reference(name, planted=False):
    """(spec, x, float64 (Y, Y_h, Y_c), float32 (Y, Y_h, Y_c)) of BAR_CASES[name], computed once; planted: with INF_AT in x"""
    spec, x = build(BAR_CASES[name])
    if planted:
        x = plant_inf(spec, x)
    return spec, x, recurrent(spec, x), recurrent(spec, x, np.float32)


def fairness(name, planted=False) -> float:
    """what float32 itself costs on a case: the worst share of the bar of the float32 restatement over Y and the tails the case reads"""
    _, _, r64, r32 = reference(name, planted)
    idx = [0] + [{"y_h": 1, "y_c": 2}[t] for t in BAR_CASES[name]["tails"]]
    return max(verdict(r32[i], r64[i]) for i in idx)
