"""InstanceNormalization and GroupNormalization without a GPU: the writer's float64 reference against torch on the CPU,
the plan of every spelling (one SpatialNorm step, its groups, the folded gamma / beta), the layouts and the plan shape the scheduler picks,
fused activations and composed per-channel arithmetic, the float16 rule, and what is refused at load."""
from __future__ import annotations

import numpy as np
import pytest

from infera_amd import onnx_writer as W


@pytest.fixture(scope="module")
def api(built):
    from infera_amd import capi

    return capi


def load_plan(api, tmp_path, blob, name="sn"):
    p = W.write(str(tmp_path / f"{name}.onnx"), blob)
    api.load_model(name, p)
    try:
        return api.get_plan(name)
    finally:
        api.unload_model(name)


def kinds(plan):
    return [s["kind"] + ("+" + s["act"] if "act" in s else "") for s in plan["plan"]["steps"]]


def norm_step(plan):
    (s,) = [s for s in plan["plan"]["steps"] if s["kind"] == "SpatialNorm"]
    return s


def bits(v):
    return np.asarray(v, np.float32).view(np.uint32).tolist()


EMBED = dict(pre=True, post=True)  # identity 1x1 layers around the layer: it then runs on channel-quad tensors


# ---- the reference -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,groups", [((2, 8, 5, 7), 8), ((2, 8, 5, 7), 2), ((3, 12, 3, 3), 4), ((2, 6, 19), 6), ((2, 6, 19), 3), ((1, 4, 9, 9), 1)])
def test_reference_is_torch(shape, groups):
    import torch
    import torch.nn.functional as F

    rng = np.random.default_rng(1)
    x, g, b = rng.normal(size=shape) * 3 + 5, rng.normal(size=shape[1]), rng.normal(size=shape[1])
    got = W.spatialnorm_reference(x, groups, g, b, 1e-5)
    want = F.group_norm(torch.from_numpy(x), groups, torch.from_numpy(g), torch.from_numpy(b), 1e-5).numpy()
    assert float(np.abs(got - want).max()) <= 1e-12
    if groups == shape[1]:
        want = F.instance_norm(torch.from_numpy(x), weight=torch.from_numpy(g), bias=torch.from_numpy(b), eps=1e-5).numpy()
        assert float(np.abs(got - want).max()) <= 1e-12


# ---- spellings ---------------------------------------------------------------------------------------------------------------------
def layer_params(spec):
    return next(p for op, out, ins, p in spec["layers"] if out == "norm")


def test_instance_norm_is_one_step(api, tmp_path):
    blob, spec = W.spatial_norm_model(8, 8, (5, 7))
    plan = load_plan(api, tmp_path, blob)
    assert kinds(plan) == ["SpatialNorm"]
    s = norm_step(plan)
    p = layer_params(spec)
    assert (s["C"], s["groups"], s["E"], s["hw"], s["in1"] if "in1" in s else -1) == (8, 8, 35, [5, 7], -1)
    assert s["scale_bits"] == bits(p["gamma"]) and s["shift_bits"] == bits(p["beta"])
    assert abs(s["epsilon"] - 1e-5) < 1e-11
    assert plan["plan"]["output_shape"] == [-1, 8, 5, 7]
    # [N, C, L] runs as [N, C, 1, L]
    s1 = norm_step(load_plan(api, tmp_path, W.spatial_norm_model(8, 8, (19,))[0]))
    assert (s1["groups"], s1["E"], s1["hw"]) == (8, 19, [1, 19])


@pytest.mark.parametrize("form,n_params", [("op18", 4), ("op21", 8)])
def test_group_norm_operator_forms(api, tmp_path, form, n_params):
    blob, spec = W.spatial_norm_model(8, 4, (5, 7), op="GroupNormalization", form=form)
    plan = load_plan(api, tmp_path, blob)
    assert kinds(plan) == ["SpatialNorm"]
    s, p = norm_step(plan), layer_params(spec)
    assert s["groups"] == 4 and s["E"] == 70
    # per-group parameters are broadcast over the group's channels at load
    assert len(s["scale_bits"]) == 8 and s["scale_bits"] == bits(p["gamma"]) and s["shift_bits"] == bits(p["beta"])
    assert len(set(s["scale_bits"])) == n_params


@pytest.mark.parametrize("affine", ["mul_add", "mul", "none"])
@pytest.mark.parametrize("back", ["const", "shape"])
def test_exporter_spelling_is_one_step_with_the_f64_fold(api, tmp_path, back, affine):
    inner = (np.asarray([0.7, 1.3], np.float32), np.asarray([0.25, -0.4], np.float32))
    blob, spec = W.spatial_norm_model(8, 2, (5, 7), op="GroupNormalization", form="exporter", inner=inner, back=back, affine=affine)
    plan = load_plan(api, tmp_path, blob)
    assert kinds(plan) == ["SpatialNorm"], kinds(plan)
    s, p = norm_step(plan), layer_params(spec)
    assert s["groups"] == 2 and s["E"] == 140 and plan["plan"]["output_shape"] == [-1, 8, 5, 7]
    # gamma'[c] = s_g gamma[c], beta'[c] = b_g gamma[c] + beta[c]: the writer's float64 values, rounded once
    assert s["scale_bits"] == bits(p["gamma"]) and s["shift_bits"] == bits(p["beta"])
    for part in ("Reshape", "InstanceNormalization") + (("Mul",) if affine != "none" else ()) + (("Add",) if affine == "mul_add" else ()):
        assert part in s["origin"]


def test_exporter_spelling_that_does_not_match_lowers_node_by_node(api, tmp_path):
    """A second reader of the normalised [N, G, E] value: no pattern; the InstanceNormalization runs on the [N, G, 1, E] tensor by its own rule."""
    net = W._DecoderNet(3)
    net.gnorm("X", 8, 2, "exporter", x_shape=(8, 5, 7), name="norm")
    net.const("flat", np.asarray([0, 8, 5, 7], np.int64))
    net.nodes.append(W.node("Reshape", ["norm_n", "flat"], ["second"], name="second_reader"))
    net.nodes.append(W.node("Add", ["norm", "second"], ["Y"], name="sum"))
    blob = W.model("two_readers", net.nodes, net.inits, [W.value_info("X", ["N", 8, 5, 7])], [W.value_info("Y", ["N", 8, 5, 7])])
    plan = load_plan(api, tmp_path, blob)
    assert kinds(plan) == ["SpatialNorm", "AffineChannel", "BinaryAct"]
    s = norm_step(plan)
    assert s["groups"] == 2 and s["hw"] == [1, 140] and s["origin"] == "InstanceNormalization:norm_inorm"


# ---- layouts, fusion, composition --------------------------------------------------------------------------------------------------
def test_plan_stays_in_channel_quads(api, tmp_path):
    plan = load_plan(api, tmp_path, W.spatial_norm_model(8, 4, (5, 7), op="GroupNormalization", **EMBED)[0])
    assert kinds(plan) == ["Conv2d", "SpatialNorm", "ConvTranspose2d"] and plan["activation_layout"] == "NC/4HW4"
    assert plan["spatialnorm"] == [{"step": 1, "kernel": "spatialnorm_fused", "groups": 4, "in_layout": "NC/4HW4", "out_layout": "NC/4HW4", "act": ""}]
    plan = load_plan(api, tmp_path, W.spatial_norm_model(8, 4, (5, 7), op="GroupNormalization")[0])
    assert plan["spatialnorm"] == [{"step": 0, "kernel": "spatialnorm_fused", "groups": 4, "in_layout": "NCHW", "out_layout": "NCHW", "act": ""}]


@pytest.mark.parametrize("act,name", [("Relu", "Relu"), ("Silu", "Swish"), ("Tanh", "Tanh"), ("Sigmoid", "Sigmoid")])
def test_activation_fuses(api, tmp_path, act, name):
    plan = load_plan(api, tmp_path, W.spatial_norm_model(8, 2, (5, 7), op="GroupNormalization", act=act, **EMBED)[0])
    assert kinds(plan) == ["Conv2d", "SpatialNorm+" + name, "ConvTranspose2d"]
    assert plan["spatialnorm"][0]["act"] == name


def test_kinds_the_convolution_epilogues_do_not_take_stay_a_step(api, tmp_path):
    plan = load_plan(api, tmp_path, W.spatial_norm_model(8, 2, (5, 7), op="GroupNormalization", act="Softplus", **EMBED)[0])
    assert kinds(plan) == ["Conv2d", "SpatialNorm", "Unary+Softplus", "ConvTranspose2d"]


@pytest.mark.parametrize("act,tail", [("Relu", ["Unary+Relu"]), ("Silu", ["Unary+Swish"])])
def test_activation_does_not_fuse_with_a_second_reader(api, tmp_path, act, tail):
    net = W._DecoderNet(3)
    n = net.inorm("X", 8, name="norm")
    a = net.silu(n) if act == "Silu" else net.act(n, act)
    out = net.add(a, n)
    blob, _ = net.finish("second_reader", W.value_info("X", ["N", 8, 5, 7]), out, ["N", 8, 5, 7], extra={})
    assert kinds(load_plan(api, tmp_path, blob)) == ["SpatialNorm"] + tail + ["BinaryAct"]


def test_per_channel_mul_add_compose(api, tmp_path):
    net = W._DecoderNet(3)
    n = net.inorm("X", 8, name="norm")
    mul, add = np.linspace(0.5, 2.0, 8).astype(np.float32), np.linspace(-1, 1, 8).astype(np.float32)
    net.nodes.append(W.node("Mul", [n, net.const("k_mul", mul.reshape(8, 1, 1))], ["m"], name="scale"))
    net.nodes.append(W.node("Add", ["m", net.const("k_add", add.reshape(1, 8, 1, 1))], ["a"], name="shift"))
    net.nodes.append(W.node("Relu", ["a"], ["Y"], name="relu"))
    blob = W.model("compose", net.nodes, net.inits, [W.value_info("X", ["N", 8, 5, 7])], [W.value_info("Y", ["N", 8, 5, 7])])
    plan = load_plan(api, tmp_path, blob)
    assert kinds(plan) == ["SpatialNorm+Relu"]
    s, p = norm_step(plan), net.layers[0][3]
    # the AffineChannel rule: each node folds in f64 and rounds (gamma * k, then beta * k, then + shift)
    g = (mul.astype(np.float64) * p["gamma"]).astype(np.float32)
    b = ((mul.astype(np.float64) * p["beta"]).astype(np.float32).astype(np.float64) + add).astype(np.float32)
    assert s["scale_bits"] == bits(g) and s["shift_bits"] == bits(b)


# ---- plan selection ----------------------------------------------------------------------------------------------------------------
FUSED, GENERAL = ["spatialnorm_fused"], ["spatialnorm_stats", "spatialnorm_apply"]
SELECTION = [
    # (C, G, hw), channel quads?, kernels
    ((8, 8, (5, 7)), True, FUSED), ((8, 4, (5, 7)), True, FUSED), ((8, 2, (5, 7)), True, FUSED), ((32, 1, (16, 16)), True, FUSED), ((8, 8, (19,)), True, FUSED),
    ((12, 4, (3, 3)), True, GENERAL), ((4, 1, (72, 72)), True, GENERAL),
    ((8, 8, (5, 7)), False, FUSED), ((8, 4, (5, 7)), False, FUSED), ((8, 2, (5, 7)), False, FUSED), ((12, 4, (3, 3)), False, FUSED), ((32, 1, (16, 16)), False, FUSED),
    ((4, 1, (64, 64)), False, FUSED), ((4, 1, (72, 72)), False, GENERAL),
]


@pytest.mark.parametrize("shape,cq,want", SELECTION)
def test_plan_selection(api, tmp_path, monkeypatch, shape, cq, want):
    c, g, hw = shape
    op = "InstanceNormalization" if g == c else "GroupNormalization"
    blob, _ = W.spatial_norm_model(c, g, hw, op=op, act="Silu", **(EMBED if cq else {}))
    monkeypatch.delenv("INFERA_SPATIALNORM_FUSED", raising=False)
    plan = load_plan(api, tmp_path, blob)
    layout = "NC/4HW4" if cq else "NCHW"
    assert [k["kernel"] for k in plan["spatialnorm"]] == want
    assert all(k["in_layout"] == layout and k["out_layout"] == layout for k in plan["spatialnorm"])
    core = [k for k in kinds(plan) if k.startswith("Spatial")]
    assert core == (["SpatialNorm+Swish"] if want == FUSED else ["SpatialStats", "SpatialNorm+Swish"])
    if want == GENERAL:
        stats, norm = [s for s in plan["plan"]["steps"] if s["kind"].startswith("Spatial")]
        assert norm["in"] == stats["in"] and norm["in1"] == stats["out"] and stats["groups"] == g
    # the knob selects the general plan everywhere and changes nothing else
    monkeypatch.setenv("INFERA_SPATIALNORM_FUSED", "0")
    off = load_plan(api, tmp_path, blob)
    assert [k["kernel"] for k in off["spatialnorm"]] == GENERAL and off["activation_layout"] == plan["activation_layout"]
    assert [k for k in kinds(off) if not k.startswith("SpatialStats")] == [k for k in kinds(plan) if not k.startswith("SpatialStats")]


def test_whole_models_stay_in_channel_quads(api, tmp_path):
    for blob, n in ((W.style_net_small()[0], 6), (W.unet_small(norm="group")[0], 5)):
        plan = load_plan(api, tmp_path, blob)
        assert plan["activation_layout"] == "NC/4HW4" and len(plan["spatialnorm"]) == n
        assert all(k["kernel"] == "spatialnorm_fused" and k["in_layout"] == "NC/4HW4" for k in plan["spatialnorm"])
        assert "Unary" not in "".join(kinds(plan))
    assert kinds(load_plan(api, tmp_path, W.unet_small(norm="group")[0])).count("SpatialNorm+Swish") == 5


# ---- float16 -----------------------------------------------------------------------------------------------------------------------
def test_float16_graph_gets_a_rounding_behind_the_step(api, tmp_path):
    g, b = np.linspace(0.5, 1.5, 8).astype(np.float16), np.linspace(-0.5, 0.5, 8).astype(np.float16)
    nodes = [W.node("InstanceNormalization", ["X", "g", "b"], ["n"], name="norm"), W.node("Relu", ["n"], ["Y"], name="relu")]
    blob = W.model("half", nodes, [W.tensor("g", g), W.tensor("b", b)], [W.value_info("X", ["N", 8, 5, 7], W.FLOAT16)], [W.value_info("Y", ["N", 8, 5, 7], W.FLOAT16)])
    plan = load_plan(api, tmp_path, blob)
    assert kinds(plan) == ["RoundHalf", "SpatialNorm+Relu", "RoundHalf"]
    assert norm_step(plan)["scale_bits"] == bits(g.astype(np.float32))


# ---- rejections --------------------------------------------------------------------------------------------------------------------
def _raw(op="InstanceNormalization", x_dims=("N", 8, 5, 7), inputs=("X", "S", "B"), n_scale=8, n_bias=8, attrs=(), opset=13, pre=()):
    inits = [W.tensor("S", np.ones(n_scale, np.float32)), W.tensor("B", np.zeros(n_bias, np.float32))]
    return W.model("bad", list(pre) + [W.node(op, list(inputs), ["Y"], list(attrs), name="norm")], inits, [W.value_info("X", list(x_dims))],
                   [W.value_info("Y", ["N"] + ["d%d" % i for i in range(len(x_dims) - 1)])], opset=opset)


_GN = dict(op="GroupNormalization", opset=18)
REJECTIONS = {
    "scale_not_constant": (dict(inputs=("X", "X", "B")), "InstanceNormalization", "scale and B must be constant"),
    "bias_not_constant": (dict(inputs=("X", "S", "X")), "InstanceNormalization", "scale and B must be constant"),
    "scale_length": (dict(n_scale=7), "InstanceNormalization", "scale / B must have C = 8 entries"),
    "bias_length": (dict(n_bias=4), "InstanceNormalization", "scale / B must have C = 8 entries"),
    "rank_2": (dict(x_dims=("N", 8)), "InstanceNormalization", "rank 3 or 4"),
    "rank_5": (dict(x_dims=("N", 8, 3, 3, 3)), "InstanceNormalization", "rank 3 or 4"),
    "E_above_2_24": (dict(x_dims=("N", 8, 4097, 4096)), "InstanceNormalization", "exceeds 2^24"),
    "groups_do_not_divide": (dict(attrs=[W.attr_i("num_groups", 3)], **_GN), "GroupNormalization", "num_groups = 3 does not divide C = 8"),
    "gn18_length_fits_neither": (dict(attrs=[W.attr_i("num_groups", 4)], n_scale=2, n_bias=2, **_GN), "GroupNormalization", "scale / bias have 2 and 2 entries"),
    "gn21_per_group_length": (dict(attrs=[W.attr_i("num_groups", 4)], n_scale=4, n_bias=4, op="GroupNormalization", opset=21), "GroupNormalization", "opset 21 takes C = 8"),
    "gn_below_opset_18": (dict(attrs=[W.attr_i("num_groups", 4)], op="GroupNormalization", opset=13), "GroupNormalization", "needs opset 18"),
}


@pytest.mark.parametrize("case", list(REJECTIONS))
def test_rejections(api, tmp_path, case):
    kw, op, why = REJECTIONS[case]
    with pytest.raises(api.InferaError) as e:
        load_plan(api, tmp_path, _raw(**kw))
    assert f"node 'norm' ({op}): unsupported operator form: " in str(e.value) and why in str(e.value), str(e.value)


def test_symbolic_spatial_extent_is_refused(api, tmp_path):
    """Only the row axis of a model's input may be symbolic, so no value with a symbolic spatial extent reaches the operator: the loader's
    own message refuses the model (the operator's check stands behind it)."""
    with pytest.raises(api.InferaError, match="only the leading .* dimension of the input may be symbolic"):
        load_plan(api, tmp_path, _raw(x_dims=("N", 8, "h", 7)))


def test_time_major_value_is_refused(api, tmp_path):
    """[N, T, F] -> Transpose(1, 0, 2) is time-major (what feeds a recurrent layer): not an [N, C, L] tensor"""
    blob = _raw(x_dims=("N", 8, 5), pre=[W.node("Transpose", ["X"], ["Xt"], [W.attr_ints("perm", [1, 0, 2])], name="tm")], inputs=("Xt", "S", "B"))
    with pytest.raises(api.InferaError) as e:
        load_plan(api, tmp_path, blob)
    assert "node 'norm' (InstanceNormalization): unsupported operator form: " in str(e.value) and "time-major" in str(e.value), str(e.value)
