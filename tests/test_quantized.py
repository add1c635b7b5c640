"""Statically quantised ONNX models without a GPU: the parser's int8 / uint8 / int32 tensors, the plans of the QDQ and QLinearMatMul
spellings, what is refused at load, and how far the integer definition of a QDense step may stand from the float
evaluation of the same QDQ graph."""
from __future__ import annotations

import numpy as np
import pytest

from infera_amd import onnx_writer as W
from infera_amd import synth

# the seeds, shapes and weight forms tests/test_quantized_gpu.py runs whole networks with
NETWORKS = [dict(dims=(128, 256, 64, 1), seed=1234), dict(dims=(30, 100, 2), seed=77, tail="Softmax"), dict(dims=(30, 100), seed=5), dict(dims=(128, 256), seed=6),
            dict(dims=(1000, 64), seed=7)]


@pytest.fixture(scope="module")
def api(built):
    from infera_amd import capi

    return capi


def load_plan(api, tmp_path, blob, name="q"):
    p = W.write(str(tmp_path / f"{name}.onnx"), blob)
    api.load_model(name, p)
    try:
        return api.get_plan(name)
    finally:
        api.unload_model(name)


def canonical(plan):
    """The steps without their origins, buffers renumbered in the order the steps meet them."""
    ids, out = {0: 0}, []
    for s in plan["plan"]["steps"]:
        s = {k: v for k, v in s.items() if k != "origin"}
        for key in ("in", "out"):
            s[key] = ids.setdefault(s[key], len(ids))
        out.append(s)
    return out


def kinds(plan):
    return [s["kind"] for s in plan["plan"]["steps"]]


@pytest.mark.parametrize("int32_data", [False, True], ids=["raw_data", "int32_data"])
@pytest.mark.parametrize("w_type,x_type", [("int8", "uint8"), ("uint8", "int8")])
def test_small_integer_tensors_round_trip(api, tmp_path, int32_data, w_type, x_type):
    spec = W.quantized_mlp_spec((30, 100, 2), x_type=x_type, w_type=w_type, w_zero_points=w_type == "uint8", seed=11)
    plan = load_plan(api, tmp_path, W.quantized_from_spec(spec, int32_data=int32_data))
    for s, L, q in zip(plan["plan"]["steps"], spec["layers"], spec["q"]):
        flat = L["wq"].reshape(-1)
        assert s["w_sum"] == int(flat.sum()) and s["w_hash"] == int((flat * (np.arange(flat.size) % 251 + 1)).sum())
        assert s["bias_sum"] == int(L["bias_q"].sum()) and s["bias"] == "int32"
        assert s["x_zero_point"] == q[1] and s["w_type"] == w_type and s["x_type"] == x_type


def test_tensor_whose_bytes_disagree_with_its_dims_is_refused(api, tmp_path):
    spec = W.quantized_mlp_spec((8, 4), seed=3)
    good = W.quantized_from_spec(spec)
    w = spec["layers"][0]["wq"].astype(np.int8)
    for int32_data in (False, True):
        ok = W.tensor("W0", w, int32_data=int32_data)
        short = W.tensor("W0", w.reshape(-1)[:-1], int32_data=int32_data)
        bad = short.replace(W._vi(1, 31), W._vi(1, 8) + W._vi(1, 4), 1)  # 31 elements under dims [8, 4]
        blob = W.quantized_from_spec(spec, int32_data=int32_data)
        assert ok in blob
        p = W.write(str(tmp_path / "bad.onnx"), blob.replace(W._ld(5, ok), W._ld(5, bad), 1))
        with pytest.raises(api.InferaError, match="element count does not match dims"):
            api.load_model("bad", p)
    assert kinds(load_plan(api, tmp_path, good)) == ["QDense"]
    # int32_data that does not fit the declared byte type
    wide = W.tensor("W0", w.astype(np.int32), int32_data=True).replace(W._vi(2, W.INT32), W._vi(2, W.INT8), 1)
    wide = wide.replace(W._varint(int(w.reshape(-1)[0])), W._varint(300), 1) if int(w.reshape(-1)[0]) >= 0 else None
    if wide is not None:
        blob = W.quantized_from_spec(spec, int32_data=True)
        p = W.write(str(tmp_path / "wide.onnx"), blob.replace(W._ld(5, W.tensor("W0", w, int32_data=True)), W._ld(5, wide), 1))
        with pytest.raises(api.InferaError, match="outside the int8 range|element count"):
            api.load_model("wide", p)


@pytest.mark.parametrize("layer", ["matmul_add", "gemm", "gemm_transb"])
@pytest.mark.parametrize("tail", ["", "Sigmoid", "Softmax"])
def test_qdq_mlp_is_three_qdense_steps(api, tmp_path, layer, tail):
    spec = W.quantized_mlp_spec((128, 256, 64, 3), tail=tail)
    plan = load_plan(api, tmp_path, W.quantized_from_spec(spec, layer=layer))
    assert kinds(plan) == ["QDense"] * 3 + ({"": [], "Sigmoid": ["Unary"], "Softmax": ["Softmax"]}[tail])
    assert [(s["K"], s["M"]) for s in plan["plan"]["steps"][:3]] == [(128, 256), (256, 64), (64, 3)]
    assert all(s["bias"] == "int32" and s["w_type"] == "int8" and s["x_type"] == s["y_type"] == "uint8" for s in plan["plan"]["steps"][:3])
    assert [s["per_channel"] for s in plan["plan"]["steps"][:3]] == [True, True, True]
    assert plan["plan"]["flops_per_row"] == 2 * (128 * 256 + 256 * 64 + 64 * 3)
    assert plan["qdense"] == [{"step": 0, "in_bytes": False, "out_bytes": True}, {"step": 1, "in_bytes": True, "out_bytes": True},
                              {"step": 2, "in_bytes": True, "out_bytes": False}]


def test_byte_buffer_knob(api, tmp_path, monkeypatch):
    monkeypatch.setenv("INFERA_QDENSE_BYTES", "0")
    plan = load_plan(api, tmp_path, W.quantized_from_spec(W.quantized_mlp_spec((128, 256, 64, 1))))
    assert all(not q["in_bytes"] and not q["out_bytes"] for q in plan["qdense"])


@pytest.mark.parametrize("x_type,per_channel", [("uint8", True), ("int8", False)])
def test_qlinear_spelling_gives_the_same_plan(api, tmp_path, x_type, per_channel):
    spec = W.quantized_mlp_spec((128, 256, 64, 1), acts=["Relu", "Relu", ""], x_type=x_type, per_channel=per_channel, bias=None)
    qdq = load_plan(api, tmp_path, W.quantized_from_spec(spec, "qdq"), "qdq")
    qlin = load_plan(api, tmp_path, W.quantized_from_spec(spec, "qlinear"), "qlin")
    assert kinds(qlin) == ["QDense"] * 3
    assert canonical(qdq) == canonical(qlin)
    assert qdq["qdense"] == qlin["qdense"]


def test_bias_forms_and_activations(api, tmp_path):
    for bias, want in (("int32", "int32"), ("f32", "f32"), (None, "none")):
        spec = W.quantized_mlp_spec((33, 31), acts=[("Clip", -0.25, 0.5)], bias=bias, x_type="int8")
        (s,) = load_plan(api, tmp_path, W.quantized_from_spec(spec))["plan"]["steps"]
        assert (s["kind"], s["bias"], s["act"]) == ("QDense", want, "Clip")
    # a Relu in front of a range that starts at 0 is that range's saturation: the step carries no activation (and equals the QLinear form)
    spec = W.quantized_mlp_spec((33, 31), acts=["Relu"])
    assert spec["q"][1][1] == 0
    (s,) = load_plan(api, tmp_path, W.quantized_from_spec(spec))["plan"]["steps"]
    assert "act" not in s
    spec["q"][1] = (spec["q"][1][0], 7)
    (s,) = load_plan(api, tmp_path, W.quantized_from_spec(spec))["plan"]["steps"]
    assert s["act"] == "Relu"


def _qdq_around(op, cols=12, scale=0.02, zp=3, dtype=np.uint8):
    inits = [W.tensor("s", np.array(scale, np.float32)), W.tensor("z", np.array(zp, dtype))]
    nodes = [W.node("QuantizeLinear", ["X", "s", "z"], ["Xq"], name="q_in"), W.node("DequantizeLinear", ["Xq", "s", "z"], ["Xd"], name="dq_in"),
             W.node(op, ["Xd"], ["H"], name="mid"), W.node("QuantizeLinear", ["H", "s", "z"], ["Hq"], name="q_out"),
             W.node("DequantizeLinear", ["Hq", "s", "z"], ["Y"], name="dq_out")]
    return W.model("qdq_" + op, nodes, inits, [W.value_info("X", ["N", cols])], [W.value_info("Y", ["N", cols])])


def test_qdq_pair_away_from_a_matmul_is_fake_quant(api, tmp_path):
    plan = load_plan(api, tmp_path, _qdq_around("Sigmoid"))
    assert kinds(plan) == ["FakeQuant", "Unary", "FakeQuant"]
    assert plan["plan"]["steps"][0]["type"] == "uint8" and plan["plan"]["steps"][0]["zero_point"] == 3


def test_weight_only_model_is_plain_dense(api, tmp_path):
    spec = W.quantized_mlp_spec((30, 100, 2), tail="Softmax")
    plan = load_plan(api, tmp_path, W.quantized_from_spec(spec, weight_only=True))
    assert "QDense" not in kinds(plan) and "FakeQuant" not in kinds(plan) and kinds(plan).count("Dense") == 2


# ---- refused at load ------------------------------------------------------------------------------------------------------------------

def _single(K=8, M=4, **edit):
    """One QDQ layer as nodes / initialisers a test can edit before it is assembled."""
    spec = W.quantized_mlp_spec((K, M), seed=3, **edit)
    return spec


def _graph(nodes, inits, K=8, M=4, out_type=W.FLOAT):
    return W.model("refuse", nodes, inits, [W.value_info("X", ["N", K])], [W.value_info("Y", ["N", M], out_type)], opset=21)


def _refused(api, tmp_path, blob, node_name, why):
    p = W.write(str(tmp_path / "refused.onnx"), blob)
    with pytest.raises(api.InferaError) as e:
        api.load_model("refused", p)
    msg = str(e.value)
    assert node_name in msg and "unsupported operator form" in msg and why in msg, msg


def test_rejections_name_their_node(api, tmp_path):
    f = lambda n, v: W.tensor(n, np.array(v, np.float32))  # noqa: E731
    u8 = lambda n, v: W.tensor(n, np.array(v, np.uint8))  # noqa: E731
    i8 = lambda n, v: W.tensor(n, np.array(v, np.int8))  # noqa: E731
    w = W.tensor("W", np.arange(32, dtype=np.int8).reshape(8, 4))
    base = [f("s", 0.1), u8("z", 0), f("ws", 0.05), i8("wz", 0), w]
    tailn = [W.node("DequantizeLinear", ["W", "ws", "wz"], ["Wd"], name="dq_w"), W.node("MatMul", ["Xd", "Wd"], ["Y"], name="mm")]
    q_in = [W.node("QuantizeLinear", ["X", "s", "z"], ["Xq"], name="q_in"), W.node("DequantizeLinear", ["Xq", "s", "z"], ["Xd"], name="dq_in")]
    # DynamicQuantizeLinear
    _refused(api, tmp_path, _graph([W.node("DynamicQuantizeLinear", ["X"], ["Xq", "xs", "xz"], name="dyn"),
                                    W.node("DequantizeLinear", ["Xq", "xs", "xz"], ["Xd"], name="dq_in")] + tailn, base), "dyn", "depend on its chunk")
    # a scale computed in the graph
    _refused(api, tmp_path, _graph([W.node("Abs", ["X"], ["sv"], name="abs"), W.node("QuantizeLinear", ["X", "sv", "z"], ["Xq"], name="q_in"),
                                    q_in[1]] + tailn, base), "q_in", "not a constant")
    # per-axis quantisation of an activation
    _refused(api, tmp_path, _graph(q_in + tailn, [W.tensor("s", np.full(8, 0.1, np.float32)), W.tensor("z", np.zeros(8, np.uint8))] + base[2:]), "q_in", "per-axis")
    # blocked quantisation
    _refused(api, tmp_path, _graph([W.node("QuantizeLinear", ["X", "s", "z"], ["Xq"], [W.attr_i("block_size", 4)], name="q_in"), q_in[1]] + tailn, base), "q_in", "block_size")
    # other element types
    _refused(api, tmp_path, _graph(q_in + tailn, [f("s", 0.1), W.tensor("z", np.array(0, np.int32))] + base[2:]), "q_in", "element type")
    _refused(api, tmp_path, _graph(q_in + tailn, base[:2] + [f("ws", 0.05), W.tensor("wz", np.array(0, np.int64)), w]), "dq_w", "element type")
    # a zero point of another type than the data
    _refused(api, tmp_path, _graph(q_in + tailn, base[:2] + [f("ws", 0.05), u8("wz", 0), w]), "dq_w", "differs from the data's")
    _refused(api, tmp_path, _graph([q_in[0], W.node("DequantizeLinear", ["Xq", "s", "z2"], ["Xd"], name="dq_in")] + tailn, base + [i8("z2", 0)]), "dq_in", "type")
    # scales that are not finite and positive
    for bad in (0.0, -0.1, float("inf"), float("nan")):
        _refused(api, tmp_path, _graph(q_in + tailn, [f("s", bad)] + base[1:]), "q_in", "finite and positive")
        _refused(api, tmp_path, _graph(q_in + tailn, base[:2] + [f("ws", bad)] + base[3:]), "dq_w", "finite and positive")
    # a quantised graph output
    _refused(api, tmp_path, _graph([W.node("QuantizeLinear", ["X", "s", "z"], ["Y"], name="q_in")], base[:2], M=8, out_type=W.UINT8), "q_in", "end the graph with DequantizeLinear")
    # K beyond what the int32 accumulator holds
    Kcap = (2 ** 31 - 1) // (255 * 255)
    for K, ok in ((Kcap, True), (Kcap + 1, False)):
        big = [f("s", 0.1), u8("z", 0), f("ws", 0.05), i8("wz", 0), W.tensor("W", np.ones((K, 2), np.int8))]
        blob = _graph(q_in + tailn, big, K=K, M=2)
        if ok:
            assert kinds(load_plan(api, tmp_path, blob)) == ["QDense"]
        else:
            _refused(api, tmp_path, blob, "mm", "beyond the cap")


@pytest.mark.parametrize("op", ["MatMulInteger", "QLinearConv", "ConvInteger"])
def test_other_integer_operators_stay_unsupported(api, tmp_path, op):
    blob = _graph([W.node(op, ["X", "X"], ["Y"], name="n0")], [])
    p = W.write(str(tmp_path / "unsup.onnx"), blob)
    with pytest.raises(api.InferaError, match="unsupported operator"):
        api.load_model("unsup", p)


# ---- the integer definition against the float evaluation of the QDQ graph ---------------------------------------------------------------

@pytest.mark.parametrize("net", NETWORKS, ids=lambda n: "x".join(map(str, n["dims"])))
def test_integer_reference_stays_within_one_step_of_the_float_graph(net):
    spec = W.quantized_mlp_spec(net["dims"], seed=net["seed"], acts=["Relu"] * (len(net["dims"]) - 2) + ["Relu" if len(net["dims"]) == 2 else ""])
    x = synth.table(net["seed"] + 100, 0, 2000, net["dims"][0])
    got = W.quantized_reference(spec, x, "int", tail=False).astype(np.float64)
    step = float(spec["q"][-1][0])
    for mode in ("f64", "f32"):
        d = np.abs(got - W.quantized_reference(spec, x, mode, tail=False).astype(np.float64)) / step
        print(net["dims"], mode, "share of differing elements", float((d > 0).mean()), "largest difference in steps", float(d.max()))
        assert float((d > 1e-3).mean()) <= 1e-3 and float(d.max()) <= 1.0 + 1e-3  # at most 1 in 1000, each by exactly one step of y_scale
