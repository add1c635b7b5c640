"""The elementwise family (hip/eltwise.hip), the activation switch (apply_act_c in hip/device_common.hpp, its copies in chain_device.inc and
mlp_device.inc) at every site that applies it, and the row kernels (softmax_small / softmax_rows<LPR, EPL> / softmax_wave, the softmax
heads fused into the dense epilogues) against the float64 definitions of tests/eltwise_ref.py -- not against the fp32 oracle, which was
written with the same formulas.  Inputs span the float32 range (SWEEP: zeros, subnormals, exact halves, the exp overflow threshold, the
float limits, +-inf, NaN); one rule decides (eltwise_ref.verdict), with no masks and no allowed share of misses.  Every case asserts
from the plan which step kind served it, and prints its worst error as a share of the bar 1e-4 |ref| + 1e-6
(profiles/eltwise_range_ratios.txt holds a run's lines).

What the lowering makes of the binary spellings (asserted below): Add / Sub / Mul with a [C] constant on either side and Div by one
become an `AffineChannel` step (affine_rows_kernel: x * scale + shift) -- Div only where every reciprocal is a normal f32; Div of a
constant, Min, Max, Pow and PRelu stay `BinaryConst` (binary_const_kernel); PRelu with the slope on the left, and Pow / PRelu against a
[N, 1] value, are refused at load."""
from __future__ import annotations

import numpy as np
import pytest

from infera_amd import onnx_writer as W
from tests import dense_ref as R
from tests import eltwise_ref as E

pytestmark = pytest.mark.gpu

ROWS = (1, 33, 257)


@pytest.fixture(scope="module")
def api(built):
    from infera_amd import capi

    assert capi.device_count() >= 1, capi.get_devices()
    return capi


class Served:
    """one loaded model"""

    def __init__(self, api, tmp_path, blob, name="eltwise_range"):
        self.api, self.name = api, name
        api.load_model(name, W.write(str(tmp_path / "m.onnx"), blob))
        self.plan = api.get_plan(name)
        self.steps = self.plan["plan"]["steps"]
        self.kinds = [s["kind"] for s in self.steps]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.api.unload_model(self.name)

    def rows(self, x):
        return self.api.predict(self.name, x)

    def blob(self, x, shape):
        return self.api.predict_from_blob(self.name, np.ascontiguousarray(x, np.float32).tobytes()).reshape(shape)

    def device(self, x, out_cols, offset=0):
        """a device-resident table in ONE launch (the host entry cuts a table into chunks), `offset` bytes past a 16-byte boundary"""
        api, dev = self.api, self.api.device_ordinal(0)
        d_in, d_out = api.DeviceBuffer(dev, x.nbytes + 16), api.DeviceBuffer(dev, x.shape[0] * out_cols * 4 + 16)
        try:
            d_in.upload(np.concatenate([np.zeros(offset // 4, np.float32), x.ravel()]))
            r, c = api.predict_device(self.name, d_in, x.shape[0], x.shape[1], d_out, in_offset_bytes=offset)
            assert r * c == x.shape[0] * out_cols, (r, c)
            return d_out.download((x.shape[0], out_cols))
        finally:
            d_in.free()
            d_out.free()


def judge(site, name, got, x, ref=None, exact=False):
    """the verdict on one result; returns the worst ratio"""
    ref = E.reference(name, x) if ref is None else ref
    ok, ratio = E.verdict_ref(got, ref, exact=exact or (name in E.UNARY and E.UNARY[name][0] in E.EXACT))
    assert ok.all(), (site, name, f"{(~ok).sum()} of {ok.size} miss", E.describe(ok, x, got, ref))
    return float(ratio.max())


def report(site, name, worst):
    print(f"{site} {name}: worst error / bar = {worst:.3f}")


def cross_table(rows, cols, values=E.FINITE, step=11, rstep=1):
    """[rows, cols] of `values`: element (r, c) is values[(rstep r + step c) mod n], so every column meets every value"""
    r, c = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    return np.ascontiguousarray(values[(rstep * r + step * c) % len(values)], np.float32)


# ---- the unary kernel -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(E.UNARY))
def test_unary_kernel_over_the_sweep(api, tmp_path, name):
    """Y = Op(X): an activation of the graph input is a Unary step.  [rows, 7] at rows 1, 2, 3, 4: n % 4 = 3, 2, 1, 0; 301: body and tail"""
    with Served(api, tmp_path, E.unary_graph(name, 7)) as m:
        assert m.kinds == ["Unary"] and m.steps[0]["act"] == E.act_name(name), m.steps
        worst = max(judge("Unary", name, m.rows(x), x) for x in (E.sweep_table(r) for r in (1, 2, 3, 4, 301)))
    report("Unary", name, worst)


@pytest.mark.parametrize("name", ["Sigmoid", "Softplus"])
def test_unary_kernel_second_grid_pass(api, tmp_path, name):
    """[4099, 513] in one launch: more than 2048 * 256 * 4 elements and n % 4 = 3 -- a second trip of the vec4 loop and a tail behind it"""
    rows, cols = 4099, 513
    assert rows * cols > 2048 * 256 * 4 and rows * cols % 4 == 3
    x = E.sweep_table(rows, cols)
    with Served(api, tmp_path, E.unary_graph(name, cols)) as m:
        assert m.kinds == ["Unary"] and m.steps[0]["act"] == name, m.steps
        report("Unary [4099, 513]", name, judge("Unary [4099, 513]", name, m.device(x, cols), x))


# ---- binaries ---------------------------------------------------------------------------------------------------------------------

CONSTS = (np.array([0.5, -3.0, 1e-20, 1e30, -1e-45, 0.0, 3e38], np.float32), np.array([-1.0, 2.5, 1e-7, -1e4, 1e-40, -0.0, -1e30], np.float32),
          np.array([2.0, -0.5, 1e-3, 8.0, -17.0, 1e4, -1e-7], np.float32))
POW_BASES = np.array([2.0, -2.0, 0.0, 0.5, 10.0, 1.0, -1.0], np.float32)


def const_kind(op, left, c):
    """what the lowering makes of X (op) c / c (op) X"""
    if op in ("Add", "Sub", "Mul"):
        return "AffineChannel"
    with np.errstate(all="ignore"):
        normal = lambda v: np.isfinite(v).all() and (np.abs(v) >= np.finfo(np.float32).tiny).all()
        if op == "Div" and not left and normal(c) and normal(np.float32(1) / c):
            return "AffineChannel"  # x * (1 / c), two roundings: inside the bar
    return "BinaryConst"


@pytest.mark.parametrize("left", [False, True], ids=["right", "left"])
@pytest.mark.parametrize("op", E.BINARY)
def test_binary_with_a_constant(api, tmp_path, op, left):
    x = cross_table(301, 7)
    if op == "PRelu" and left:
        with pytest.raises(api.InferaError, match="PRelu needs a constant slope"):
            api.load_model("refused", W.write(str(tmp_path / "m.onnx"), E.binary_const_graph(op, CONSTS[0], 7, left=True)))
        return
    worst = 0.0
    for c in (E.POW_EXPONENTS,) if op == "Pow" and not left else (POW_BASES,) if op == "Pow" else CONSTS:
        with Served(api, tmp_path, E.binary_const_graph(op, c, 7, left=left)) as m:
            assert m.kinds == [const_kind(op, left, c)], (m.kinds, c)
            ref = E.binary64(op, c, x) if left else E.binary64(op, x, c)
            worst = max(worst, judge(m.kinds[0], op, m.rows(x), x, ref))
    report("constant " + ("left" if left else "right"), op, worst)


def test_min_max_prelu_against_a_constant_at_nan(api, tmp_path):
    """the NaN table: fminf / fmaxf return the constant, PRelu's product is NaN"""
    nan = np.full((5, 7), np.nan, np.float32)
    for op in ("Min", "Max", "PRelu"):
        for left in (False, True) if op != "PRelu" else (False,):
            with Served(api, tmp_path, E.binary_const_graph(op, CONSTS[2], 7, left=left)) as m:
                got = m.rows(nan)
                assert m.kinds == ["BinaryConst"] and (np.isnan(got).all() if op == "PRelu" else (got == CONSTS[2]).all()), (op, left, got[0])


@pytest.mark.parametrize("op", E.BINARY)
def test_binary_of_two_tensors(api, tmp_path, op):
    """binary_act_kernel: 301 * 7 elements, n % 4 = 3"""
    a = cross_table(301, 7)
    b = cross_table(301, 7, E.POW_EXPONENTS if op == "Pow" else E.FINITE, step=3, rstep=5)
    with Served(api, tmp_path, E.binary_tensor_graph(op, 7)) as m:
        assert m.kinds == ["SliceCols", "SliceCols", "BinaryAct"] and "row_scalar" not in m.steps[2], m.steps
        report("two tensors", op, judge("BinaryAct", op, m.rows(np.concatenate([a, b], axis=1)), a, E.binary64(op, a, b)))


@pytest.mark.parametrize("swap", [False, True], ids=["right", "left"])
@pytest.mark.parametrize("op", E.BINARY)
def test_binary_with_a_row_scalar(api, tmp_path, op, swap):
    """binary_rowscalar_kernel: [N, 7] against a [N, 1] value; Pow and PRelu have no such form and are refused"""
    blob = E.binary_tensor_graph(op, 7, 1, swap=swap)
    if op in ("Pow", "PRelu"):
        with pytest.raises(api.InferaError, match="equal shapes"):
            api.load_model("refused", W.write(str(tmp_path / "m.onnx"), blob))
        return
    a, b = cross_table(301, 7), cross_table(301, 1, rstep=5)
    with Served(api, tmp_path, blob) as m:
        assert m.kinds == ["SliceCols", "SliceCols", "BinaryAct"] and m.steps[2]["row_scalar"] == ("left" if swap and op in ("Sub", "Div") else "right"), m.steps
        ref = E.binary64(op, b, a) if swap else E.binary64(op, a, b)
        report("row scalar " + ("left" if swap else "right"), op, judge("BinaryAct", op, m.rows(np.concatenate([a, b], axis=1)), a, ref))


def _pow2(rng, n):
    return np.ldexp(rng.choice([-1.0, 1.0], n), rng.integers(-3, 4, n)).astype(np.float32)


INDEX_SHAPES = ((80000, 7), (5300, 100), (4100, 516))
INDEX_FORMS = ("Mul", "Add", "Mul+Add", "Max", "PRelu", "Div-left")


@pytest.mark.parametrize("shape", INDEX_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("form", INDEX_FORMS)
def test_running_row_position_past_the_first_grid_pass(api, tmp_path, form, shape):
    """binary_const_kernel and affine_rows_kernel keep the position inside the row (j += stride % per_row, then a wrap), which matters from
    the second trip of the grid-stride loop: more than 2048 * 256 work items in one launch, per_row no divisor of the stride.  Multipliers
    are powers of two and addends small integers, so x * 2^e + c rounds once whether or not it is contracted; a quotient and a comparison
    round once or not at all: equality with float32(float64 result).  Mul, Add and the Mul -> Add pair are AffineChannel steps with S == 1
    (16-byte pieces where C % 4 == 0: 100 and 516; one float each at 7, and at 100 behind a pointer 4 bytes off a 16-byte boundary), the
    rest BinaryConst"""
    rows, C = shape
    rng = np.random.default_rng([rows, C])
    x = (rng.standard_normal((rows, C)) * np.ldexp(1.0, rng.integers(-6, 7, (rows, C)))).astype(np.float32)
    mul, add, pos = _pow2(rng, C), rng.integers(-8, 9, C).astype(np.float32), np.abs(_pow2(rng, C))
    x64 = x.astype(np.float64)
    blob, kind, ref = {
        "Mul": (E.binary_const_graph("Mul", mul, C), "AffineChannel", x64 * mul),
        "Add": (E.binary_const_graph("Add", add, C, left=True), "AffineChannel", x64 + add),
        "Mul+Add": (E.binary_const_graph(["Mul", "Add"], [mul, add], C), "AffineChannel", x64 * mul + add),
        "Max": (E.binary_const_graph("Max", add / 8, C), "BinaryConst", np.maximum(x64, add / 8)),
        "PRelu": (E.binary_const_graph("PRelu", pos, C), "BinaryConst", np.where(x64 >= 0, x64, x64 * pos)),
        "Div-left": (E.binary_const_graph("Div", add + 9, C, left=True), "BinaryConst", (add.astype(np.float64) + 9) / x64),
    }[form]
    want = ref.astype(np.float32)
    with Served(api, tmp_path, blob) as m:
        assert m.kinds == [kind], m.steps
        vec4 = kind == "AffineChannel" and C % 4 == 0
        assert rows * C // (4 if vec4 else 1) > 2048 * 256 or (rows, C) == (5300, 100)
        if not vec4 or (rows, C) != (5300, 100):  # (100-float rows in 16-byte pieces fit one pass)
            assert (2048 * 256) % (C // 4 if vec4 else C) != 0
        assert np.array_equal(m.device(x, C), want), (form, shape, "aligned")
        if (rows, C) == (5300, 100):
            assert np.array_equal(m.device(x, C, offset=4), want), (form, shape, "4 bytes off")


# ---- activations in epilogues -----------------------------------------------------------------------------------------------------

def act_rows(rows, K):
    """rows of FINITE (an infinity times a zero weight is NaN), the last of several all NaN"""
    x = cross_table(rows, K)
    if rows > 1:
        x[-1] = np.nan
    return x


def compose64(acts, x, srcs):
    """the float64 activations on the exact selections: layer l copies h[:, srcs[l]] and applies acts[l]"""
    h = np.asarray(x, np.float64)
    for name, src in zip(acts, srcs):
        h = h[:, src]
        with np.errstate(all="ignore"):
            v = E.UNARY[name][2](h)
        op = E.UNARY[name][0]
        h = np.where(np.isnan(h), E.NAN_TABLE[op], v) if op in E.NAN_TABLE else v
    return h


def dense_blob(dims, acts):
    srcs, nodes, inits, cur = [], [], [], "X"
    for l, (k, mm) in enumerate(zip(dims[:-1], dims[1:])):
        w, src = E.select01(k, mm)
        srcs.append(src)
        inits += [W.tensor(f"W{l}", w), W.tensor(f"B{l}", np.zeros(mm, np.float32))]
        nodes.append(W.node("Gemm", [cur, f"W{l}", f"B{l}"], [f"H{l}"]))
        out = "Y" if l == len(dims) - 2 else f"A{l}"
        nodes += E.unary_nodes(acts[l], f"H{l}", out, inits)
        cur = out
    return W.model("act_sites", nodes, inits, [W.value_info("X", ["N", dims[0]])], [W.value_info("Y", ["N", dims[-1]])]), srcs


# one (K, M) per dense.hip family, the tiled kernel, and 5 -> 17: a one-layer chain for the kinds the chain kernel takes (1 .. 5), dense_kernel else
DENSE_SITES = [(3, 5), (33, 16), (1024, 7), (128, 10), (129, 33), (24, 32), (36, 65), (5, 17)]


@pytest.mark.parametrize("name", E.MFMA_FUSABLE)
@pytest.mark.parametrize("dims", DENSE_SITES, ids=lambda d: "x".join(map(str, d)))
def test_activation_behind_a_dense_layer(api, tmp_path, dims, name):
    """a 0/1 selection with zero bias: each output copies one input, exact in any summation order, so the activation reads the input to the bit"""
    blob, srcs = dense_blob(dims, [name])
    K, M = dims
    with Served(api, tmp_path, blob) as m:
        assert m.kinds[-1] == "Dense" and m.steps[-1]["act"] == E.act_name(name), m.steps
        what = R.served_by(dims)
        if dims == (5, 17) and name in ("HardSigmoid", "HardSwish", "Swish"):
            what = "dense_kernel"  # (the chain kernel takes the kinds 1 .. 5)
        if what in ("chain_fused", "dense_tiled"):
            assert m.plan["exec"][-1] == what, m.plan["exec"]
        else:
            assert m.plan["exec"][-1] == "normal" and m.plan["dense_kernels"][0].startswith(what), (m.plan["exec"], m.plan.get("dense_kernels"))
        worst = 0.0
        for rows in ROWS + ((R.BIG,) if R.big_rows(dims) else ()):  # (dense_narrow16s_kernel from 4096 rows)
            x = act_rows(rows, K)
            worst = max(worst, judge(what, name, m.rows(x), x[:, srcs[0]], compose64([name], x, srcs)))
    report(f"Dense {K}x{M} ({what})", name, worst)


CHAIN_ACTS = [("Relu", "Sigmoid"), ("Sigmoid", "Tanh"), ("Tanh", "LeakyRelu"), ("LeakyRelu", "Clip"), ("Clip", "Relu")]


@pytest.mark.parametrize("acts", CHAIN_ACTS, ids="-".join)
def test_activations_inside_the_chain_kernel(api, tmp_path, acts):
    """chain_device.inc's own copy of the switch, kinds 1 .. 5 behind the first and behind the last layer"""
    dims = (9, 20, 4)
    blob, srcs = dense_blob(dims, acts)
    with Served(api, tmp_path, blob) as m:
        assert m.plan["exec"][0] == "chain_fused" and [s.get("act") for s in m.steps] == [E.act_name(a) for a in acts], (m.plan["exec"], m.steps)
        worst = 0.0
        for rows in ROWS:
            x = act_rows(rows, dims[0])
            ref = compose64(acts, x, srcs)
            worst = max(worst, judge("chain_fused", "-".join(acts), m.rows(x), ref, ref))
    report("chain 9x20x4", "-".join(acts), worst)


@pytest.mark.parametrize("acts", [("Sigmoid", "Tanh", "Relu"), ("Relu", "Sigmoid", "Tanh")], ids="-".join)
def test_activations_inside_the_fused_mlp(api, tmp_path, acts):
    """mlp_device.inc's copy: the parameter-free kinds 1 .. 3"""
    dims = (128, 256, 64, 1)
    blob, srcs = dense_blob(dims, acts)
    with Served(api, tmp_path, blob) as m:
        assert m.plan["exec"][0] == "mlp3_fused" and [s.get("act") for s in m.steps] == list(acts), (m.plan["exec"], m.steps)
        worst = 0.0
        for rows in ROWS:
            x = act_rows(rows, dims[0])
            ref = compose64(acts, x, srcs)
            worst = max(worst, judge("mlp3_fused", "-".join(acts), m.rows(x), ref, ref))
    report("fused MLP 128x256x64x1", "-".join(acts), worst)


def conv_blob(op, C, M, hw, name):
    w, src = E.select01(C, M)
    wt = np.ascontiguousarray(w.T if op == "Conv" else w).reshape((M, C, 1, 1) if op == "Conv" else (C, M, 1, 1))
    inits = [W.tensor("W", wt), W.tensor("B", np.zeros(M, np.float32))]
    nodes = [W.node(op, ["X", "W", "B"], ["H"])] + E.unary_nodes(name, "H", "Y", inits)
    return W.model("act_conv", nodes, inits, [W.value_info("X", ["N", C, *hw])], [W.value_info("Y", ["N", M, *hw])]), src


def run_conv_site(api, tmp_path, op, kind, geom, name):
    C, M, hw = geom
    blob, src = conv_blob(op, C, M, hw, name)
    with Served(api, tmp_path, blob) as m:
        assert m.kinds == [kind] and m.steps[0]["act"] == E.act_name(name), m.steps
        worst = 0.0
        for rows in (1, 33):
            x = act_rows(rows, C * hw[0] * hw[1]).reshape(rows, C, *hw)
            got = m.blob(x, (rows, M, *hw))
            worst = max(worst, judge(kind, name, got, x[:, src]))
        report(f"{kind} {C}->{M} {hw[0]}x{hw[1]} ({m.plan['exec'][0]})", name, worst)


@pytest.mark.parametrize("name", E.MFMA_FUSABLE)
@pytest.mark.parametrize("geom", [(5, 6, (3, 5)), (32, 32, (4, 4))], ids=["5to6", "32to32"])
def test_activation_behind_a_1x1_convolution(api, tmp_path, geom, name):
    run_conv_site(api, tmp_path, "Conv", "Conv2d", geom, name)


@pytest.mark.parametrize("name", E.KINDS_1_TO_5)
@pytest.mark.parametrize("geom", [(5, 6, (3, 5)), (32, 32, (4, 4))], ids=["5to6", "32to32"])
def test_activation_behind_a_1x1_transposed_convolution(api, tmp_path, geom, name):
    run_conv_site(api, tmp_path, "ConvTranspose", "ConvTranspose2d", geom, name)


@pytest.mark.parametrize("name", E.KINDS_1_TO_5)
def test_activation_behind_a_half_dense_layer(api, tmp_path, name):
    """HDense: r = half(act(float(r))) on half inputs.  The activation's own error is held to the bar; the rounding to half that follows
    adds at most half an ulp of half: 2^-11 |ref| on normal halves, 2^-25 below them"""
    K, M = 33, 16
    w, src = E.select01(K, M)
    with np.errstate(over="ignore"):
        halves = E.FINITE.astype(np.float16)
    halves = halves[np.isfinite(halves)].astype(np.float32)
    attrs = E.UNARY[name][1]
    act = {"LeakyRelu": ("LeakyRelu", attrs.get("alpha")), "Clip": ("Clip", attrs.get("min"), attrs.get("max"))}.get(name, name)
    spec = {"dims": (K, M), "layers": [{"w": w.astype(np.float16), "b": None, "act": W._as_act(act)}], "tail": "", "grid": False, "q": None, "seed": 0}
    with Served(api, tmp_path, W.half_from_spec(spec)) as m:
        assert "HDense" in m.kinds and m.steps[m.kinds.index("HDense")]["act"] == name, m.steps
        worst = 0.0
        for rows in ROWS:
            x = cross_table(rows, K, halves)
            if rows > 1:
                x[-1] = np.nan
            got, ref = m.rows(x), E.reference(name, x[:, src])
            nan = np.isnan(ref)
            assert np.array_equal(np.isnan(got), nan), (name, rows)
            err, bar = np.abs(got.astype(np.float64) - ref)[~nan], (E.RTOL * np.abs(ref) + E.ATOL + 2.0 ** -11 * np.abs(ref) + 2.0 ** -25)[~nan]
            assert np.isfinite(got[~nan]).all() and (err <= bar).all(), (name, rows, float((err / bar).max()))
            worst = max(worst, float((err / bar).max()))
    report("HDense 33x16 (bar + half an ulp of half)", name, worst)


# ---- row kernels ------------------------------------------------------------------------------------------------------------------

LENGTHS = (3, 5, 16, 17, 64, 65, 128, 129, 256, 257, 1024, 1025, 3000)
WINDOWS = ((3, 1), (7, 3), (8, 5))  # (first row, rows): 1, 3 and 5 vectors -- a wave's last vectors are missing at 4, 2 and 1 vectors per wave


@pytest.mark.parametrize("length", LENGTHS)
@pytest.mark.parametrize("op", ["Softmax", "LogSoftmax", "NormL1", "NormL2", "NormMAX"])
def test_row_kernels(api, tmp_path, op, length):
    """one lane per row (3), every softmax_rows_kernel instance on both sides of its switch (5 .. 1024), the wave kernel (1025, 3000);
    67 rows cycling through the regimes, then 1, 3 and 5 of them"""
    x, names = E.row_batch(op, length)
    with Served(api, tmp_path, E.row_graph(op, length)) as m:
        assert m.kinds == ["Softmax"], m.steps
        worst = 0.0
        for first, rows in ((0, len(x)),) + WINDOWS:
            xs, ns = x[first:first + rows], names[first:first + rows]
            zeroed = xs.copy()
            zeroed[E.poisoned(ns)] = 0
            worst = max(worst, E.check_rows(op, xs, ns, m.rows(xs), m.rows(zeroed)))
    report(f"rows of {length}", op, worst)


def test_softmax_over_an_inner_axis(api, tmp_path):
    """Softmax over C of [N, 5, 2, 3] (opset 13): the vector's elements are 6 floats apart -- softmax_small_kernel with inner = 6"""
    blob = W.model("inner", [W.node("Softmax", ["X"], ["Y"], [W.attr_i("axis", 1)])], [], [W.value_info("X", ["N", 5, 2, 3])], [W.value_info("Y", ["N", 5, 2, 3])], opset=13)
    v, names = E.softmax_rows(5, rows=6 * 13)
    x = np.ascontiguousarray(v.reshape(13, 2, 3, 5).transpose(0, 3, 1, 2))
    with Served(api, tmp_path, blob) as m:
        assert m.kinds == ["Softmax"], m.steps
        got = m.blob(x, x.shape)
    back = np.ascontiguousarray(got.transpose(0, 2, 3, 1)).reshape(-1, 5)
    # (isolation is the row kernels' test: here the result stands in for the clean run)
    report("inner axis [N, 5, 2, 3]", "Softmax", E.check_rows("Softmax", v, names, back, back.copy()))


HEADS = [c for c in R.EPILOGUES if c[2] != "columns"] + [("chain_fused", (9, 20, 4), "rows")]


@pytest.mark.parametrize("head", ["Softmax", "LogSoftmax"])
@pytest.mark.parametrize("case", HEADS, ids=lambda c: R.case_id(c) + "-" + c[2])
def test_fused_softmax_heads(api, tmp_path, case, head):
    """exec kind dense_softmax behind a selection-matrix layer -- the logits are the inputs exactly -- in every dense.hip family that carries
    the softmax epilogue, and the chain kernel's head (the max subtraction is written out in each); regimes (a) - (e) and (g)"""
    what, dims, where = case
    srcs = [E.select01(k, mm)[1] for k, mm in zip(dims[:-1], dims[1:])]
    layers = [(E.select01(k, mm)[0], None) for k, mm in zip(dims[:-1], dims[1:])]
    rows = R.BIG if where == "big" else 257
    x, names = E.softmax_rows(dims[0], rows=rows, regimes=E.HEAD_REGIMES)
    logits = compose64(["Relu"] * (len(dims) - 2), x, srcs[:-1])[:, srcs[-1]]
    ref = E.softmax64(logits, log=head == "LogSoftmax")
    with Served(api, tmp_path, R.graph(layers, head=head)) as m:
        if what == "chain_fused":
            assert m.plan["exec"][0] == "chain_fused" and m.kinds[-1] == "Softmax", (m.plan["exec"], m.kinds)
        else:
            assert m.plan["exec"] == ["dense_softmax", "skipped"] and m.plan["dense_kernels"][0].startswith(R.family(1 << 20, *dims, 1)), (m.plan["exec"], m.plan["dense_kernels"])
        worst = 0.0
        for r in (rows,) if where == "big" else ROWS:
            got = m.rows(x[:r])
            worst = max(worst, judge(what, head, got, logits[:r], ref[:r]))
            equal = np.array([n[0] == "d" for n in names[:r]])
            if head == "Softmax":  # (behind the chain's Relu the row of -1e30 is a row of zeros: still all equal)
                assert (got[equal] == np.float32(1) / np.float32(dims[-1])).all(), (what, dims, r)
    report(f"{head} head {'x'.join(map(str, dims))} ({what}, {where})", head, worst)
