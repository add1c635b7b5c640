"""Statically quantised convolutions without a GPU: the plans of the QDQ and QLinearConv spellings, what keeps the
float path, what is refused at load, and how far the integer definition of the writer's nets stands from the float evaluation of the
same QDQ graphs."""
from __future__ import annotations

import numpy as np
import pytest

from infera_amd import onnx_writer as W
from infera_amd import synth


@pytest.fixture(scope="module")
def api(built):
    from infera_amd import capi

    return capi


def load_plan(api, tmp_path, blob, name="qc"):
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


@pytest.mark.parametrize("geom", [dict(k=1), dict(k=3, pads=1), dict(k=7, stride=2, pads=3), dict(k=3, dilation=2), dict(k=3, pads=(0, 1, 2, 1))],
                         ids=["1x1", "3x3", "7x7s2", "dilated", "asymmetric"])
@pytest.mark.parametrize("x_type,per_channel,bias", [("uint8", True, "int32"), ("int8", False, None)])
def test_both_spellings_of_a_layer_give_one_qconv_step(api, tmp_path, geom, x_type, per_channel, bias):
    spec = W.quantized_conv_spec("layer", (5, 9, 9), m=7, act="Relu" if x_type == "uint8" else "", x_type=x_type, per_channel=per_channel, bias=bias, **geom)
    qdq = load_plan(api, tmp_path, W.quantized_conv_from_spec(spec, "qdq"), "qdq")
    qlin = load_plan(api, tmp_path, W.quantized_conv_from_spec(spec, "qlinear"), "qlin")
    assert kinds(qdq) == kinds(qlin) == ["QConv2d"]
    assert canonical(qdq) == canonical(qlin)
    assert qdq["qconv"] == qlin["qconv"]
    (s,) = qdq["plan"]["steps"]
    wq, op = spec["ops"][0]["wq"], spec["ops"][0]
    assert (s["K"], s["M"], s["C"], s["k"]) == (5 * wq.shape[2] * wq.shape[3], 7, 5, list(wq.shape[2:]))
    assert s["pads"] == list(op["pads"]) and s["strides"] == list(op["strides"]) and s["dilations"] == list(op["dilations"])
    assert s["bias"] == (bias or "none") and s["x_type"] == s["y_type"] == x_type and s["per_channel"] == per_channel
    assert s["w_sum"] == int(wq.sum()) and s["x_zero_point"] == spec["q"]["X"][1]
    assert qdq["plan"]["flops_per_row"] == 2 * s["K"] * 7 * s["out_hw"][0] * s["out_hw"][1]
    # qW is [K, M] with k = (c, ky, kx): the hash over that order
    flat = np.ascontiguousarray(wq.reshape(7, -1).T).reshape(-1)
    assert s["w_hash"] == int((flat * (np.arange(flat.size) % 251 + 1)).sum())


def test_conv1d_and_bias_forms(api, tmp_path):
    for bias, want in (("int32", "int32"), ("f32", "f32"), (None, "none")):
        spec = W.quantized_conv_spec("layer", (5, 11), m=6, k=3, pads=1, act=("Clip", -0.25, 0.5), bias=bias, x_type="int8")
        plan = load_plan(api, tmp_path, W.quantized_conv_from_spec(spec))
        (s,) = plan["plan"]["steps"]
        assert (s["kind"], s["bias"], s["act"], s["k"], s["in_hw"], s["out_hw"]) == ("QConv2d", want, "Clip", [1, 3], [1, 11], [1, 11])
        assert plan["plan"]["output_shape"] == [-1, 6, 11]
    spec = W.quantized_conv_spec("layer", (5, 11), m=6, k=3, pads=1, act="", bias="int32")
    assert canonical(load_plan(api, tmp_path, W.quantized_conv_from_spec(spec, "qlinear"))) == canonical(load_plan(api, tmp_path, W.quantized_conv_from_spec(spec)))


@pytest.fixture(scope="module")
def resnet():
    return W.quantized_conv_spec("resnet", (3, 32, 32), width=8, seed=77)


@pytest.mark.parametrize("form", ["qdq", "qlinear"])
def test_residual_net_runs_on_integer_steps_in_channel_quads(api, tmp_path, resnet, form):
    plan = load_plan(api, tmp_path, W.quantized_conv_from_spec(resnet, form))
    ks = kinds(plan)
    assert "Conv2d" not in ks and "Dense" not in ks and ks.count("QConv2d") == 6 and ks.count("QDense") == 1
    assert ks[0] == "QConv2d" and ks.count("BinaryAct") == 2 and ks.count("Pool2d") == 1
    # what is left of the QuantizeLinear / DequantizeLinear pairs: the rounding of values a float step (MaxPool, Add, the global pool) made
    # or reads; never one in front of an integer layer alone
    st = plan["plan"]["steps"]
    readers = {}
    for s in st:
        for key in ("in", "in1"):
            if key in s:
                readers.setdefault(s[key], []).append(s["kind"])
    for s in st:
        if s["kind"] == "FakeQuant":
            assert any(k not in ("QConv2d", "QDense") for k in readers.get(s["out"], [])), (s, readers.get(s["out"]))
    assert plan["activation_layout"] == "NC/4HW4"
    assert [q["in_layout"] for q in plan["qconv"]] == ["NCHW"] + ["NC/4HW4"] * 5 and all(q["out_layout"] == "NC/4HW4" for q in plan["qconv"])


@pytest.mark.parametrize("groups", [4, 8], ids=["grouped", "depthwise"])
def test_grouped_layers_keep_the_float_convolution(api, tmp_path, groups):
    spec = W.quantized_conv_spec("layer", (8, 9, 9), m=8, k=3, pads=1, groups=groups, act="Relu")
    for form in ("qdq", "qlinear"):
        plan = load_plan(api, tmp_path, W.quantized_conv_from_spec(spec, form))
        assert kinds(plan) == ["FakeQuant", "Conv2d", "FakeQuant"], form
        assert plan["plan"]["steps"][2]["scale"] == pytest.approx(float(spec["q"]["C0"][0])) and plan["plan"]["steps"][2]["zero_point"] == spec["q"]["C0"][1]


def test_weight_only_and_batchnorm_keep_the_float_convolution(api, tmp_path):
    spec = W.quantized_conv_spec("layer", (4, 9, 9), m=8, k=3, pads=1)
    assert kinds(load_plan(api, tmp_path, W.quantized_conv_from_spec(spec, weight_only=True))) == ["Conv2d"]
    # QDQ conv -> BatchNormalization: folded into FLOAT weights, not into integer ones
    f = lambda n, v: W.tensor(n, np.array(v, np.float32))  # noqa: E731
    inits = [f("s", 0.1), W.tensor("z", np.array(0, np.uint8)), f("ws", 0.05), W.tensor("wz", np.array(0, np.int8)),
             W.tensor("Wt", np.ones((4, 4, 1, 1), np.int8))] + [f(n, np.full(4, v)) for n, v in (("g", 1.5), ("b", 0.1), ("mu", 0.2), ("var", 2.0))]
    nodes = [W.node("QuantizeLinear", ["X", "s", "z"], ["Xq"]), W.node("DequantizeLinear", ["Xq", "s", "z"], ["Xd"]),
             W.node("DequantizeLinear", ["Wt", "ws", "wz"], ["Wd"]), W.node("Conv", ["Xd", "Wd"], ["C"], name="conv"),
             W.node("BatchNormalization", ["C", "g", "b", "mu", "var"], ["Y"], name="bn")]
    plan = load_plan(api, tmp_path, W.model("bn", nodes, inits, [W.value_info("X", ["N", 4, 5, 5])], [W.value_info("Y", ["N", 4, 5, 5])]))
    assert kinds(plan) == ["FakeQuant", "Conv2d"] and "BatchNormalization" in plan["plan"]["steps"][1]["origin"]


def test_fake_quant_no_longer_keeps_a_float_cnn_out_of_channel_quads(api, tmp_path):
    """A QDQ graph whose convolutions stay float (grouped ones) behind a pooled head: the FakeQuant steps are layout-free."""
    spec = W.quantized_conv_spec("layer", (8, 9, 9), m=8, k=3, pads=1, groups=2, act="Relu", pooled=True)
    plan = load_plan(api, tmp_path, W.quantized_conv_from_spec(spec))
    assert kinds(plan)[:3] == ["FakeQuant", "Conv2d", "FakeQuant"] and plan["activation_layout"] == "NC/4HW4"


# ---- refused at load ------------------------------------------------------------------------------------------------------------------

def _refused(api, tmp_path, blob, node_name, why):
    p = W.write(str(tmp_path / "refused.onnx"), blob)
    with pytest.raises(api.InferaError) as e:
        api.load_model("refused", p)
    msg = str(e.value)
    assert f"node '{node_name}' (" in msg and "unsupported operator form" in msg and why in msg, msg


def _qlinear_graph(edit=None, n_inputs=9, C=4, M=6, k=3, extra_nodes=(), x_in="Xq", out_type=W.FLOAT):
    f = lambda n, v: W.tensor(n, np.array(v, np.float32))  # noqa: E731
    u8 = lambda n, v: W.tensor(n, np.array(v, np.uint8))  # noqa: E731
    inits = {"xs": f("xs", 0.1), "xz": u8("xz", 3), "w": W.tensor("w", np.ones((M, C, k, k), np.int8)), "ws": f("ws", np.full(M, 0.05)),
             "wz": W.tensor("wz", np.zeros(M, np.int8)), "ys": f("ys", 0.2), "yz": u8("yz", 0), "B": W.tensor("B", np.arange(M, dtype=np.int32))}
    inits.update(edit or {})
    ins = [x_in, "xs", "xz", "w", "ws", "wz", "ys", "yz", "B"][:n_inputs]
    nodes = [W.node("QuantizeLinear", ["X", "xs0", "xz0"], ["Xq"], name="q_in")] + list(extra_nodes) + [
        W.node("QLinearConv", ins, ["Yq"], [W.attr_ints("pads", [1, 1, 1, 1])], name="qc"), W.node("DequantizeLinear", ["Yq", "ys", "yz"], ["Y"], name="dq_out")]
    inits.setdefault("xs0", f("xs0", 0.1))
    inits.setdefault("xz0", u8("xz0", 3))
    return W.model("refuse", nodes, [v for v in inits.values() if v is not None], [W.value_info("X", ["N", C, 5, 5])], [W.value_info("Y", ["N", M, 5, 5], out_type)])


def test_qlinearconv_rejections_name_their_node(api, tmp_path):
    f = lambda n, v: W.tensor(n, np.array(v, np.float32))  # noqa: E731
    assert kinds(load_plan(api, tmp_path, _qlinear_graph())) == ["QConv2d"]
    assert kinds(load_plan(api, tmp_path, _qlinear_graph(n_inputs=8))) == ["QConv2d"]  # (B is optional)
    _refused(api, tmp_path, _qlinear_graph(n_inputs=7), "qc", "eight inputs")
    # scales, zero points or weights computed in the graph
    absn = lambda out: [W.node("Abs", ["X"], [out], name="abs")]  # noqa: E731
    _refused(api, tmp_path, _qlinear_graph({"ws": None}, extra_nodes=absn("ws")), "qc", "scale is not a constant")
    _refused(api, tmp_path, _qlinear_graph({"ys": None}, extra_nodes=absn("ys")), "qc", "scale is not a constant")
    _refused(api, tmp_path, _qlinear_graph({"xs": None}, extra_nodes=absn("xs")), "qc", "scale is not a constant")
    _refused(api, tmp_path, _qlinear_graph({"wz": None}, extra_nodes=absn("wz")), "qc", "zero point is not a constant")
    _refused(api, tmp_path, _qlinear_graph({"w": None}, extra_nodes=absn("w")), "qc", "constant kernel")
    # x_scale / x_zero_point other than the input's own
    _refused(api, tmp_path, _qlinear_graph({"xs": f("xs", 0.11)}), "qc", "differ from what input x was quantised with")
    _refused(api, tmp_path, _qlinear_graph({"xz": W.tensor("xz", np.array(4, np.uint8))}), "qc", "differ from what input x was quantised with")
    _refused(api, tmp_path, _qlinear_graph(x_in="X"), "qc", "must be a quantised activation")
    # a weight scale that is neither per tensor nor per output channel
    _refused(api, tmp_path, _qlinear_graph({"ws": f("ws", np.full(4, 0.05)), "wz": W.tensor("wz", np.zeros(4, np.int8))}), "qc", "one value or one per output channel")
    # the type rules
    _refused(api, tmp_path, _qlinear_graph({"wz": W.tensor("wz", np.zeros(6, np.uint8))}), "qc", "differs from the data's")
    _refused(api, tmp_path, _qlinear_graph({"B": f("B", np.zeros(6))}), "qc", "int32 bias")
    _refused(api, tmp_path, _qlinear_graph({"ys": f("ys", 0.0)}), "qc", "finite and positive")
    _refused(api, tmp_path, _qlinear_graph({"w": W.tensor("w", np.ones((6, 4, 3, 3), np.int32)), "wz": W.tensor("wz", np.zeros(6, np.int32))}), "qc", "element type")
    # a QDQ conv whose per-axis scale has the wrong length is refused where it is dequantised
    inits = [f("s", 0.1), W.tensor("z", np.array(0, np.uint8)), f("ws", np.full(3, 0.05)), W.tensor("wz", np.zeros(3, np.int8)), W.tensor("Wt", np.ones((6, 4, 3, 3), np.int8))]
    nodes = [W.node("QuantizeLinear", ["X", "s", "z"], ["Xq"]), W.node("DequantizeLinear", ["Xq", "s", "z"], ["Xd"]),
             W.node("DequantizeLinear", ["Wt", "ws", "wz"], ["Wd"], [W.attr_i("axis", 0)], name="dq_w"), W.node("Conv", ["Xd", "Wd"], ["Y"], name="conv")]
    _refused(api, tmp_path, W.model("refuse", nodes, inits, [W.value_info("X", ["N", 4, 5, 5])], [W.value_info("Y", ["N", 6, 3, 3])]), "dq_w", "does not match the axis")


@pytest.mark.parametrize("op", ["MatMulInteger", "ConvInteger"])
def test_the_other_integer_operators_stay_unsupported(api, tmp_path, op):
    blob = W.model("unsup", [W.node(op, ["X", "X"], ["Y"], name="n0")], [], [W.value_info("X", ["N", 8])], [W.value_info("Y", ["N", 4])])
    with pytest.raises(api.InferaError, match="unsupported operator"):
        api.load_model("unsup", W.write(str(tmp_path / "unsup.onnx"), blob))


def _cap_graph(form, C, k, hw):
    f = lambda n, v: W.tensor(n, np.array(v, np.float32))  # noqa: E731
    inits = [f("s", 0.1), W.tensor("z", np.array(0, np.uint8)), f("ws", 0.05), W.tensor("wz", np.array(0, np.int8)), W.tensor("Wt", np.ones((2, C, k, k), np.int8)), f("ys", 1.0)]
    q_in = W.node("QuantizeLinear", ["X", "s", "z"], ["Xq"], name="q_in")
    if form == "qlinear":
        nodes = [q_in, W.node("QLinearConv", ["Xq", "s", "z", "Wt", "ws", "wz", "ys", "z"], ["Yq"], name="conv"), W.node("DequantizeLinear", ["Yq", "ys", "z"], ["Y"])]
    else:
        nodes = [q_in, W.node("DequantizeLinear", ["Xq", "s", "z"], ["Xd"]), W.node("DequantizeLinear", ["Wt", "ws", "wz"], ["Wd"], name="dq_w"),
                 W.node("Conv", ["Xd", "Wd"], ["Y"], name="conv")]
    o = hw - k + 1
    return W.model("cap", nodes, inits, [W.value_info("X", ["N", C, hw, hw])], [W.value_info("Y", ["N", 2, o, o])])


@pytest.mark.parametrize("form", ["qdq", "qlinear"])
def test_k_at_and_beyond_the_accumulator_cap(api, tmp_path, form):
    assert 1321 * 25 == (2 ** 31 - 1) // (255 * 255) == 33025
    plan = load_plan(api, tmp_path, _cap_graph(form, 1321, 5, 5))
    assert kinds(plan) == ["QConv2d"] and plan["plan"]["steps"][0]["K"] == 33025
    _refused(api, tmp_path, _cap_graph(form, 33026, 1, 5), "conv", "beyond the cap")


# ---- the integer definition against the float evaluation of the QDQ graph ---------------------------------------------------------------

# the shapes and seeds tests/test_quantized_conv_gpu.py runs (a sample of its single layers, and its residual net)
LAYERS = [dict(in_shape=(17, 5, 7), m=17, k=3, pads=1, seed=700), dict(in_shape=(64, 9, 9), m=33, k=3, pads=1, seed=701), dict(in_shape=(3, 9, 9), m=4, k=7, stride=2, pads=3, seed=702),
          dict(in_shape=(64, 9, 9), m=17, k=1, seed=703), dict(in_shape=(4, 63), m=4, k=3, pads=1, seed=704), dict(in_shape=(17, 9, 9), m=33, k=3, dilation=2, seed=705)]


def _one_step(a, b, step):
    d = np.abs(a.astype(np.float64) - b.astype(np.float64)) / step
    print("share of differing elements", float((d > 0).mean()), "largest difference in steps", float(d.max()))
    return float((d > 1e-3).mean()) <= 1e-3 and float(d.max()) <= 1.0 + 1e-3  # at most 1 in 1000, each by exactly one step of y_scale


@pytest.mark.parametrize("layer", LAYERS, ids=lambda l: "C%d_M%d_k%s" % (l["in_shape"][0], l["m"], l["k"]))
def test_integer_reference_of_a_layer_stays_within_one_step_of_the_float_graph(layer):
    spec = W.quantized_conv_spec("layer", act="Relu", **layer)
    n = int(np.prod(layer["in_shape"]))
    x = synth.table(layer["seed"] + 100, 0, 64, n).reshape([64] + list(layer["in_shape"]))
    assert _one_step(W.quantized_conv_reference(spec, x, "int"), W.quantized_conv_reference(spec, x, "f64"), float(spec["q"]["C0"][0]))


def test_integer_reference_of_the_residual_net_stays_within_one_step_of_the_float_graph(resnet):
    x = synth.table(177, 0, 200, 3 * 32 * 32).reshape(200, 3, 32, 32)
    assert _one_step(W.quantized_conv_reference(resnet, x, "int"), W.quantized_conv_reference(resnet, x, "f64"), float(resnet["q"]["fc"][0]))
