"""ConvNeXt's norm over the channel axis and the channels-last detour around it, without a GPU: what the
lowering recognises -- Transpose(0,2,3,1) of a tensor a step wrote as a view that moves nothing, LayerNormalization on it as one ChannelNorm
step, MatMul on it as a 1x1 Conv2d, Hugging Face's channels-first chain as the same step --, what it folds, which kernel form and layout the
scheduler reports, and what it refuses.  Every plan test here needs the ChannelNorm step: before it, the loads were refused."""
from __future__ import annotations

import struct

import numpy as np
import pytest

from infera_amd import onnx_writer as W

SPELLINGS = ("nhwc_op", "layernorm2d", "channels_first")
REGS_MAX_C = 512  # host/channelnorm.hpp kChannelNormRegsMaxC


@pytest.fixture(scope="module")
def api(built):
    from infera_amd import capi

    return capi


def plan_of(api, tmp_path, blob, name="cn"):
    api.load_model(name, W.write(str(tmp_path / f"{name}.onnx"), blob))
    try:
        return api.get_plan(name)
    finally:
        api.unload_model(name)


def kinds(plan):
    return [s["kind"] for s in plan["plan"]["steps"]]


def norms(plan):
    return [s for s in plan["plan"]["steps"] if s["kind"] == "ChannelNorm"]


def bits(v):
    return [struct.unpack("<I", struct.pack("<f", float(f)))[0] for f in np.asarray(v, np.float32).reshape(-1)]


def refused(api, tmp_path, blob, *words):
    from infera_amd.capi import InferaError

    with pytest.raises(InferaError) as e:
        plan_of(api, tmp_path, blob, "refused")
    for w in words:
        assert w in str(e.value), (w, str(e.value))


# ---- the reference ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 8, 5, 7), (3, 12, 3, 3), (1, 4, 1, 1), (2, 6, 1, 19)])
def test_reference_is_torch_layer_norm_over_the_permuted_tensor(shape):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(1)
    x, g, b = rng.uniform(-2, 2, shape), rng.uniform(0.5, 1.5, shape[1]), rng.uniform(-1, 1, shape[1])
    want = torch.nn.functional.layer_norm(torch.from_numpy(x).permute(0, 2, 3, 1), (shape[1],), torch.from_numpy(g), torch.from_numpy(b), 1e-6).permute(0, 3, 1, 2).numpy()
    assert np.abs(W.channelnorm_reference(x, g, b, 1e-6) - want).max() <= 1e-12
    want = torch.nn.functional.layer_norm(torch.from_numpy(x).permute(0, 2, 3, 1), (shape[1],), torch.from_numpy(g), None, 1e-6).permute(0, 3, 1, 2).numpy()
    assert np.abs(W.channelnorm_reference(x, g, None, 1e-6) - want).max() <= 1e-12


# ---- spellings -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("front", ["relu", "conv"])
def test_three_spellings_one_step(api, tmp_path, front):
    got = []
    for sp in SPELLINGS:
        blob, spec = W.channel_norm_model(8, (5, 7), spelling=sp, front=front)
        plan = plan_of(api, tmp_path, blob)
        assert kinds(plan) == (["Unary", "ChannelNorm"] if front == "relu" else ["Conv2d", "ChannelNorm", "ConvTranspose2d"]), (sp, kinds(plan))
        (s,) = norms(plan)
        assert (s["C"], s["hw"], "act" in s) == (8, [5, 7], False)
        assert s["scale_bits"] == bits(spec["gamma"]) and s["shift_bits"] == bits(spec["beta"])
        assert s["epsilon"] == pytest.approx(1e-6, rel=1e-6)
        got.append((s["C"], s["hw"], s["epsilon"], s["scale_bits"], s["shift_bits"]))
    assert got[0] == got[1] == got[2]


@pytest.mark.parametrize("spelling", SPELLINGS)
def test_square_spelled_as_mul_and_no_bias(api, tmp_path, spelling):
    blob, spec = W.channel_norm_model(6, (3, 3), spelling=spelling, square="mul", bias=False)
    (s,) = norms(plan_of(api, tmp_path, blob))
    assert s["scale_bits"] == bits(spec["gamma"]) and s["shift_bits"] == []


@pytest.mark.parametrize("act", ["Relu", "Sigmoid"])
@pytest.mark.parametrize("spelling", SPELLINGS)
def test_trailing_mul_add_and_activation_fold(api, tmp_path, spelling, act):
    """Mul / Add per channel behind the norm compose into gamma and beta -- an f64 product rounded per node --, and the activation is the step's"""
    blob, spec = W.channel_norm_model(12, (3, 3), spelling=spelling, act=act, post_affine=True)
    plan = plan_of(api, tmp_path, blob)
    assert kinds(plan) == ["Unary", "ChannelNorm"]
    (s,) = norms(plan)
    g, b, (g2, b2) = spec["gamma"], spec["beta"], spec["post"]
    scale = (g2.astype(np.float64) * g.astype(np.float64)).astype(np.float32)
    shift = (g2.astype(np.float64) * b.astype(np.float64)).astype(np.float32)  # (the Mul)
    shift = (shift.astype(np.float64) + b2.astype(np.float64)).astype(np.float32)  # (the Add)
    assert s["scale_bits"] == bits(scale) and s["shift_bits"] == bits(shift)
    assert s["act"] == act


# ---- layouts and forms -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [3, 4, 5, 6, 8, 96])
def test_layouts(api, tmp_path, c):
    plan = plan_of(api, tmp_path, W.channel_norm_model(c, (2, 3), front="relu")[0])
    assert [(k["in_layout"], k["out_layout"]) for k in plan["channelnorm"]] == [("NCHW", "NCHW")]
    plan = plan_of(api, tmp_path, W.channel_norm_model(c, (2, 3), front="conv")[0])
    want = "NC/4HW4" if c % 4 == 0 else "NCHW"
    assert [(k["in_layout"], k["out_layout"]) for k in plan["channelnorm"]] == [(want, want)]
    assert plan["activation_layout"] == want


@pytest.mark.parametrize("front", ["relu", "conv"])
def test_kernel_form(api, tmp_path, monkeypatch, front):
    monkeypatch.delenv("INFERA_CHANNELNORM_REGS", raising=False)
    for c, want in ((8, "channelnorm_regs"), (REGS_MAX_C, "channelnorm_regs"), (REGS_MAX_C + 4, "channelnorm_reread"), (768, "channelnorm_reread")):
        plan = plan_of(api, tmp_path, W.channel_norm_model(c, (1, 2), front=front)[0])
        assert [k["kernel"] for k in plan["channelnorm"]] == [want], (c, plan["channelnorm"])
    monkeypatch.setenv("INFERA_CHANNELNORM_REGS", "0")  # (read when a model is loaded)
    plan = plan_of(api, tmp_path, W.channel_norm_model(8, (1, 2), front=front)[0])
    assert [k["kernel"] for k in plan["channelnorm"]] == ["channelnorm_reread"]


# ---- blocks ----------------------------------------------------------------------------------------------------------------------------
def conv_tables(api, tmp_path, blob):
    """(plan, [per step: its reported fields but the buffer numbers and the node names])"""
    plan = plan_of(api, tmp_path, blob)
    return plan, [{k: v for k, v in s.items() if k not in ("in", "out", "in1", "origin")} for s in plan["plan"]["steps"]]


@pytest.mark.parametrize("gelu", ["op", "decomposed"])
@pytest.mark.parametrize("layer_scale", [True, False])
def test_blocks_lower_as_the_nchw_block(api, tmp_path, gelu, layer_scale):
    """The torchvision and Hugging Face blocks -- permute, LayerNorm, Linear, GELU, Linear, layer scale, permute back -- give the step list
    of the same block spelled with the channels-first norm and 1x1 Conv nodes: kinds, fused activations, where layer scale and the residual
    land, and every step's reported fields (the ChannelNorm's gamma and beta bits among them; a Conv2d step reports its geometry, not its
    weights: that the weights and biases are the same numbers is what tests/test_channel_norm_gpu.py shows, bit for bit).  The Gelu operator is a Unary pass behind
    the first 1x1 convolution in all three: the convolution epilogues take Relu .. Clip and the mobile-net gates, not Gelu (plan.hpp
    mfma_fusable), for a Conv node as for this MatMul.  The decomposed Erf GELU keeps its passes."""
    plans = {st: conv_tables(api, tmp_path, W.convnext_block_model(8, (7, 7), style=st, gelu=gelu, layer_scale=layer_scale)[0]) for st in ("nchw", "torchvision", "hf")}
    ref_plan, ref_steps = plans["nchw"]
    want = ["Conv2d", "Conv2d", "ChannelNorm", "Conv2d"] + (["Unary"] if gelu == "op" else ["AffineChannel", "AffineChannel", "BinaryAct", "AffineChannel"]) + \
           ["Conv2d", "BinaryAct", "ConvTranspose2d"]
    assert kinds(ref_plan) == want
    if gelu == "op":
        assert ref_plan["plan"]["steps"][4]["act"] == "Gelu"
    for st in ("torchvision", "hf"):
        plan, steps = plans[st]
        assert kinds(plan) == want, st
        assert steps == ref_steps, st
        assert plan["exec"] == ref_plan["exec"] and plan["activation_layout"] == ref_plan["activation_layout"] == "NC/4HW4"
        for key in ("channelnorm", "residual_fused", "conv_precision"):
            assert plan.get(key) == ref_plan.get(key), (st, key)


# ---- the whole model -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("style", ["torchvision", "hf", "nchw"])
def test_small_convnext(api, tmp_path, style):
    spec = W.convnext_spec()
    plan = plan_of(api, tmp_path, W.convnext_from_spec(spec, style=style))
    assert kinds(plan).count("ChannelNorm") == W.convnext_norm_count(spec) == 5
    assert "ChannelShuffle" not in kinds(plan) and "LayerNorm" not in kinds(plan)
    assert plan["plan"]["output_shape"] == [-1, spec["classes"]]
    assert plan["activation_layout"] == "NC/4HW4"
    assert all(k["kernel"] == "channelnorm_regs" and k["in_layout"] == "NC/4HW4" for k in plan["channelnorm"][:-1])
    assert [(s["C"], s["hw"]) for s in norms(plan)] == [(8, [8, 8]), (8, [8, 8]), (8, [8, 8]), (16, [4, 4]), (16, [1, 1])]


def test_small_convnext_in_float16(api, tmp_path):
    spec = W.convnext_spec()
    plan = plan_of(api, tmp_path, W.convnext_from_spec(spec, style="torchvision", half=True))
    k = kinds(plan)
    at = [i for i, s in enumerate(k) if s == "ChannelNorm"]
    assert len(at) == 5 and all(k[i + 1] == "RoundHalf" for i in at), k
    assert plan["plan"]["output_shape"] == [-1, spec["classes"]]


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def view_graph(tail, inits=(), out="Y", out_dims=("N", 4, 3, 3), c=4, extra_outputs=()):
    """Relu(X) -> Transpose(0,2,3,1) = "v" [N,3,3,c], then `tail`"""
    nodes = [W.node("Relu", ["X"], ["r"], name="front"), W.node("Transpose", ["r"], ["v"], [W.attr_ints("perm", [0, 2, 3, 1])], name="to_last")] + list(tail)
    f32 = lambda name, v: W.tensor(name, np.asarray(v, np.float32))  # noqa: E731
    base = [f32("g", np.ones(c)), f32("b", np.zeros(c))]
    return W.model("refused", nodes, base + list(inits), [W.value_info("X", ["N", c, 3, 3])], [W.value_info(out, list(out_dims))] + list(extra_outputs), opset=20)


BACK = W.node("Transpose", ["t"], ["Y"], [W.attr_ints("perm", [0, 3, 1, 2])], name="to_first")


def test_refusals(api, tmp_path):
    f32 = lambda name, v: W.tensor(name, np.asarray(v, np.float32))  # noqa: E731
    ln = lambda ins, outs=("t",), axis=-1, name="norm": W.node("LayerNormalization", list(ins), list(outs), [W.attr_i("axis", axis), W.attr_f("epsilon", 1e-6)], name=name)  # noqa: E731
    # a view as the graph output
    refused(api, tmp_path, view_graph([ln(["v", "g", "b"], ["Y"])], out_dims=("N", 3, 3, 4)), "node 'norm' (LayerNormalization)", "unsupported operator form", "channels-last view", "graph output")
    # Softmax on a view
    refused(api, tmp_path, view_graph([W.node("Softmax", ["v"], ["t"], [W.attr_i("axis", -1)], name="sm"), BACK]), "node 'sm' (Softmax)", "unsupported operator form", "channels-last view")
    # a view plus an NCHW value
    refused(api, tmp_path, view_graph([W.node("Add", ["v", "r"], ["t"], name="mixed"), BACK]), "node 'mixed' (Add)", "unsupported operator form", "mixes the channels-last view")
    # MatMul of a view by an activation (the search for attention patterns, which runs before the walk, names it)
    refused(api, tmp_path, view_graph([W.node("MatMul", ["v", "v"], ["t"], name="mm"), BACK]), "node 'mm' (MatMul)", "unsupported operator form", "constant weight matrix")
    # MatMul by a constant of the wrong shape
    refused(api, tmp_path, view_graph([W.node("MatMul", ["v", "w"], ["t"], name="mm"), BACK], [f32("w", np.ones((3, 4)))]), "node 'mm' (MatMul)", "constant f32 [4, M]")
    # Scale of the wrong length
    refused(api, tmp_path, view_graph([ln(["v", "g5", "b"]), BACK], [f32("g5", np.ones(5))]), "node 'norm' (LayerNormalization)", "unsupported operator form", "C = 4")
    # a per-channel constant of another length
    refused(api, tmp_path, view_graph([W.node("Mul", ["v", "g5"], ["t"], name="scale"), BACK], [f32("g5", np.ones(5))]), "node 'scale' (Mul)", "unsupported operator form", "per channel")
    # LayerNormalization over another axis
    refused(api, tmp_path, view_graph([ln(["v", "g", "b"], axis=-2), BACK]), "node 'norm' (LayerNormalization)", "unsupported operator form", "axis = -1", "got axis -2")
    # a consumed Mean
    tail = [ln(["v", "g", "b"], ["t0", "mu"]), W.node("Add", ["t0", "mu"], ["t"], name="uses_mean"), BACK]
    refused(api, tmp_path, view_graph(tail), "node 'norm' (LayerNormalization)", "unsupported operator form", "Mean is consumed")
    # another Transpose of a view
    refused(api, tmp_path, view_graph([W.node("Transpose", ["v"], ["Y"], [W.attr_ints("perm", [0, 2, 1, 3])], name="again")], out_dims=("N", 3, 3, 4)), "node 'again' (Transpose)", "Transpose(0,3,1,2)")


def test_c_beyond_the_cap_is_refused(api, tmp_path):
    refused(api, tmp_path, W.channel_norm_model(4097, (1, 1), front="relu")[0], "LayerNormalization", "unsupported operator form", "C = 4097", "4096")


def test_transpose_of_a_model_input_keeps_its_message(api, tmp_path):
    nodes = [W.node("Transpose", ["X"], ["v"], [W.attr_ints("perm", [0, 2, 3, 1])], name="to_last"), W.node("Relu", ["v"], ["Y"], name="act")]
    blob = W.model("input_view", nodes, [], [W.value_info("X", ["N", 4, 3, 3])], [W.value_info("Y", ["N", 3, 3, 4])], opset=20)
    refused(api, tmp_path, blob, "node 'to_last' (Transpose)", "only the channel shuffle")


def test_channels_first_chain_with_a_second_reader_keeps_its_message(api, tmp_path):
    """the centred value d is read by a third node: no norm is recognised, and the first ReduceMean is refused as before"""
    net = W._ConvNextNet()
    cur = net.op("Relu", ["X"], "front")
    cur = net.norm_first(cur, np.ones(4), np.zeros(4), 1e-6, "norm")
    net.op("Add", [cur, "norm_d"], "Y", name="second_reader")
    blob = W.model("second_reader", net.nodes, net.inits, [W.value_info("X", ["N", 4, 3, 3])], [W.value_info("Y", ["N", 4, 3, 3])], opset=20)
    refused(api, tmp_path, blob, "node 'norm_mean' (ReduceMean)", "axes must be exactly the spatial axes")
