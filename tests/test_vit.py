"""Vision Transformers without a GPU: what the loader recognises as the Tokens step (Conv -> Flatten(2) / Reshape -> Transpose(0,2,1) ->
Concat(class tokens) -> Add(position table)), the plans it makes of ViT-shaped models, and what it refuses."""
import os

import numpy as np
import pytest

from infera_amd import onnx_writer as W


@pytest.fixture(scope="module")
def api(built):
    from infera_amd import capi

    return capi


def plan_of(api, tmp_path, blob, name="vit"):
    path = W.write(os.path.join(str(tmp_path), name + ".onnx"), blob)
    api.load_model(name, path)
    try:
        return api.get_plan(name)
    finally:
        api.unload_model(name)


def load_error(api, tmp_path, blob, name="bad"):
    path = W.write(os.path.join(str(tmp_path), name + ".onnx"), blob)
    with pytest.raises(Exception) as e:
        api.load_model(name, path)
        api.unload_model(name)
    return str(e.value)


def canon(plan):
    """The steps without origins, buffers renumbered in order of first appearance (tests/test_transformer.py)."""
    ids, out = {}, []
    for s in plan["plan"]["steps"]:
        t = {k: v for k, v in s.items() if k != "origin"}
        for k in ("in", "in1", "in2", "out"):
            if k in t:
                t[k] = ids.setdefault(t[k], len(ids))
        out.append(t)
    return out


def kinds(plan):
    return [s["kind"] for s in plan["plan"]["steps"]]


def tokens_step(plan):
    (s,) = [s for s in plan["plan"]["steps"] if s["kind"] == "Tokens"]
    return s


LAYER = ["LayerNorm", "Dense", "Attention", "Dense", "BinaryAct", "LayerNorm", "Dense", "Unary", "Dense", "BinaryAct"]


def test_the_step_alone_loads(api, tmp_path):
    p = plan_of(api, tmp_path, W.tokens_model(8, (4, 5), prefix=1, pos=True)[0])
    assert kinds(p) == ["Unary", "Tokens"]
    s = tokens_step(p)
    assert (s["C"], s["S"], s["prefix"], s["pos"], s["T"], s["E"]) == (8, 20, 1, True, 21, 8)
    assert p["plan"]["output_shape"] == [-1, 21, 8]
    s = tokens_step(plan_of(api, tmp_path, W.tokens_model(5, (7,), view="none")[0]))  # an [N, C, L] tensor is the view itself
    assert (s["C"], s["S"], s["prefix"], s["pos"], s["T"], s["E"]) == (5, 7, 0, False, 7, 5)


def test_small_vit_plan(api, tmp_path):
    spec = W.vit_spec()
    p = plan_of(api, tmp_path, W.vit_from_spec(spec))
    assert kinds(p) == ["Conv2d", "Tokens"] + LAYER * 2 + ["LayerNorm", "SliceCols", "Dense"], kinds(p)
    assert "CopyCols" not in kinds(p) and "BinaryConst" not in kinds(p)
    assert all(a["packed_qkv"] for a in p["plan"]["steps"] if a["kind"] == "Attention")
    s = tokens_step(p)
    assert (s["C"], s["S"], s["prefix"], s["pos"], s["T"], s["E"]) == (32, 16, 1, True, 17, 32)
    assert p["plan"]["output_shape"] == [-1, 5]
    # the stem model: two convolutions, the crossing, one layer, the mean over time
    q = plan_of(api, tmp_path, W.cnn_stem_encoder_from_spec(W.cnn_stem_encoder_spec()))
    assert kinds(q)[:3] == ["Conv2d", "Conv2d", "Tokens"] and kinds(q)[-2:] == ["MeanTime", "Dense"] and tokens_step(q)["prefix"] == 0


@pytest.mark.parametrize("prefix", [1, 2])
def test_one_plan_for_every_spelling(api, tmp_path, prefix):
    spec = W.vit_spec(img=(3, 8, 12), prefix=prefix, layers=1)
    want = canon(plan_of(api, tmp_path, W.vit_from_spec(spec, batch=3, expand="literal")))
    assert tokens_step(plan_of(api, tmp_path, W.vit_from_spec(spec)))["prefix"] == prefix
    for view in ("flatten", "reshape", "shape_subgraph"):
        for expand in ("subgraph", "literal"):
            assert canon(plan_of(api, tmp_path, W.vit_from_spec(spec, view=view, expand=expand, batch=3))) == want, (view, expand)
    # a symbolic batch: the same steps
    sym = [canon(plan_of(api, tmp_path, W.vit_from_spec(spec, view=view))) for view in ("flatten", "reshape", "shape_subgraph")]
    assert sym[0] == sym[1] == sym[2] and [s["kind"] for s in sym[0]] == [s["kind"] for s in want]
    # a batch fixed at 1 takes the [1, p, E] constant as it stands
    one = plan_of(api, tmp_path, W.vit_from_spec(spec, expand="none", batch=1))
    assert tokens_step(one)["tables_hash"] == tokens_step(plan_of(api, tmp_path, W.vit_from_spec(spec)))["tables_hash"]
    # the tables are part of the plan: another class token, another hash
    other = dict(spec, cls=spec["cls"] + np.float32(1))
    assert tokens_step(plan_of(api, tmp_path, W.vit_from_spec(other)))["tables_hash"] != tokens_step(one)["tables_hash"]


def test_position_add_with_a_second_reader_stays_a_step(api, tmp_path):
    spec = W.vit_spec()
    fused, unfused = plan_of(api, tmp_path, W.vit_from_spec(spec)), plan_of(api, tmp_path, W.vit_from_spec(spec, second_reader=True))
    assert kinds(unfused)[:4] == ["Conv2d", "Tokens", "BinaryConst", "BinaryAct"], kinds(unfused)
    s = tokens_step(unfused)
    assert s["pos"] is False and s["prefix"] == 1 and s["T"] == 17
    assert unfused["plan"]["flops_per_row"] == fused["plan"]["flops_per_row"] > 0
    two = plan_of(api, tmp_path, W.tokens_model(8, (4, 5), prefix=1, pos=True, second_reader=True)[0])
    assert kinds(two) == ["Unary", "Tokens", "BinaryConst", "BinaryAct"] and two["plan"]["flops_per_row"] == 0


def test_both_input_layouts_occur(api, tmp_path):
    on_input = plan_of(api, tmp_path, W.tokens_model(8, (4, 5), front="relu")[0])
    assert on_input["tokens"] == [{"step": 1, "kernel": "tokens_nchw", "in_layout": "NCHW"}]
    quads = plan_of(api, tmp_path, W.tokens_model(8, (4, 5), front="conv")[0])
    assert quads["activation_layout"] == "NC/4HW4" and quads["tokens"] == [{"step": 1, "kernel": "tokens_cq", "in_layout": "NC/4HW4"}]
    # a convolution the scheduler cannot keep in quads (6 channels): the step reads NCHW
    assert plan_of(api, tmp_path, W.tokens_model(6, (4, 5), front="conv")[0])["tokens"][0]["in_layout"] == "NCHW"
    vit = plan_of(api, tmp_path, W.vit_from_spec(W.vit_spec()))
    assert vit["tokens"][0]["in_layout"] == "NC/4HW4" and vit["exec"][0] != "conv2d_generic", vit["exec"]


def test_decomposed_gelu_keeps_its_passes(api, tmp_path):
    spec = W.vit_spec(layers=1)
    op, dec = plan_of(api, tmp_path, W.vit_from_spec(spec)), plan_of(api, tmp_path, W.vit_from_spec(spec, gelu="decomposed"))
    assert len(kinds(dec)) == len(kinds(op)) + 3 and kinds(dec).count("AffineChannel") == 3 and kinds(dec).count("Tokens") == 1


def test_float16_graph_keeps_the_position_add(api, tmp_path):
    """Movement is exact on halves; the sum is rounded to half by its own steps."""
    c, hw, h = 8, (4, 5), np.float16
    inits = [W.tensor("cls", np.ones((1, 1, c), h)), W.tensor("pos", (np.arange(21 * c) % 7).reshape(1, 21, c).astype(h)), W.tensor("view", np.asarray([0, c, 20], np.int64))]
    nodes = [W.node("Relu", ["X"], ["front"]), W.node("Reshape", ["front", "view"], ["v"]), W.node("Transpose", ["v"], ["t"], [W.attr_ints("perm", [0, 2, 1])]),
             W.node("Concat", ["cls", "t"], ["cat"], [W.attr_i("axis", 1)]), W.node("Add", ["cat", "pos"], ["emb"], name="pos_add")]
    blob = W.model("tokens16", nodes, inits, [W.value_info("X", [1, c] + list(hw), W.FLOAT16)], [W.value_info("emb", [1, 21, c], W.FLOAT16)], opset=13)
    p = plan_of(api, tmp_path, blob)
    assert kinds(p) == ["RoundHalf", "Unary", "Tokens", "BinaryConst", "RoundHalf"], kinds(p)  # (the first rounds the f32 input of a call)
    assert tokens_step(p)["pos"] is False and tokens_step(p)["prefix"] == 1


# ---- refusals: each names its node ----------------------------------------------------------------------------------------------------
def _tokens_graph(c, hw, prefix, pos, **kw):
    nodes, inits = [W.node("Relu", ["X"], ["front"], name="front_relu")], []
    out = W.token_nodes(nodes, inits, "front", c, hw, prefix, pos, **kw)
    T = int(np.prod(hw)) + sum(len(p) for p in (prefix or ()))
    return W.model("tokens", nodes, inits, [W.value_info("X", ["N", c] + list(hw))], [W.value_info(out, ["N", T, c])], opset=13)


def test_refusals(api, tmp_path):
    c, hw = 8, (4, 5)
    rows = lambda p, w=c: np.ones((p, w), np.float32)  # noqa: E731
    msg = load_error(api, tmp_path, _tokens_graph(c, hw, [rows(1)], None, prefix_behind=True))
    assert "node 'tok_concat' (Concat): unsupported operator form:" in msg and "behind the tokens" in msg, msg
    msg = load_error(api, tmp_path, _tokens_graph(c, hw, [rows(1, c + 1)], None))
    assert "node 'tok_concat' (Concat): unsupported operator form:" in msg and "9 wide" in msg and "E = 8" in msg, msg
    msg = load_error(api, tmp_path, _tokens_graph(c, hw, [rows(1)], np.ones((25, c), np.float32)))
    assert "node 'tok_pos_add' (Add)" in msg and "[1,25,8]" in msg, msg
    msg = load_error(api, tmp_path, _tokens_graph(c, hw, [rows(17)], None))
    assert "node 'tok_concat' (Concat): unsupported operator form:" in msg and "cap of 16" in msg, msg
    msg = load_error(api, tmp_path, _tokens_graph(c, hw, [rows(1)], None, expand="none"))  # a symbolic batch needs the Expand
    assert "node 'tok_concat' (Concat): unsupported operator form:" in msg and "not expanded" in msg, msg
    # a non-constant prefix: two token values joined
    nodes, inits = [W.node("Relu", ["X"], ["fa"]), W.node("Neg", ["X"], ["fb"])], []
    a = W.token_nodes(nodes, inits, "fa", c, hw, p="a_")
    b = W.token_nodes(nodes, inits, "fb", c, hw, p="b_")
    nodes.append(W.node("Concat", [a, b], ["both"], [W.attr_i("axis", 1)], name="join"))
    msg = load_error(api, tmp_path, W.model("two", nodes, inits, [W.value_info("X", ["N", c] + list(hw))], [W.value_info("both", ["N", 40, c])], opset=13))
    assert "node 'join' (Concat): unsupported operator form:" in msg and "not a constant" in msg, msg
    # Concat on another axis
    nodes, inits = [W.node("Relu", ["X"], ["front"])], [W.tensor("k", np.ones((1, 20, 2), np.float32))]
    t = W.token_nodes(nodes, inits, "front", c, hw)
    nodes.append(W.node("Concat", ["k", t], ["wide"], [W.attr_i("axis", 2)], name="widen"))
    msg = load_error(api, tmp_path, W.model("ax", nodes, inits, [W.value_info("X", [1, c] + list(hw))], [W.value_info("wide", [1, 20, c + 2])], opset=13))
    assert "node 'widen' (Concat): unsupported operator form:" in msg and "axis = 2" in msg, msg
    # the caps of the kernel
    msg = load_error(api, tmp_path, _tokens_graph(2, (1 << 11, 1 << 10), None, None))
    assert "node 'tok_transpose' (Transpose): unsupported operator form:" in msg and "cap of 1048576" in msg, msg
    msg = load_error(api, tmp_path, _tokens_graph(65537, (1, 2), None, None))
    assert "node 'tok_transpose' (Transpose): unsupported operator form:" in msg and "C = 65537 channels, above the cap of 65536" in msg, msg
    # (a crossing that moves nothing is an alias without caps; the class-token Concat that makes it a step meets them)
    msg = load_error(api, tmp_path, _tokens_graph(65537, (1, 1), [rows(1, 65537)], None))
    assert "node 'tok_concat' (Concat): unsupported operator form:" in msg and "C = 65537 channels, above the cap of 65536" in msg, msg
    # a symbolic spatial extent is the loader's to refuse
    nodes, inits = [W.node("Relu", ["X"], ["front"])], []
    t = W.token_nodes(nodes, inits, "front", c, (4, 5), view="shape_subgraph")
    msg = load_error(api, tmp_path, W.model("sym", nodes, inits, [W.value_info("X", ["N", c, "H", 5])], [W.value_info(t, ["N", "S", c])], opset=13))
    assert "only the leading (row/batch) dimension of the input may be symbolic, got" in msg, msg


def test_unchanged_behaviour(api, tmp_path):
    # Transpose(0,2,1) of the model input (or a view of it) moves data no step wrote: refused as before
    nodes = [W.node("Transpose", ["X"], ["Y"], [W.attr_ints("perm", [0, 2, 1])], name="swap")]
    msg = load_error(api, tmp_path, W.model("t", nodes, [], [W.value_info("X", ["N", 4, 6])], [W.value_info("Y", ["N", 6, 4])], opset=13))
    assert "node 'swap' (Transpose)" in msg and "would need data moved" in msg, msg
    inits = [W.tensor("shape", np.asarray([0, 4, 6], np.int64))]
    nodes = [W.node("Reshape", ["X", "shape"], ["V"]), W.node("Transpose", ["V"], ["Y"], [W.attr_ints("perm", [0, 2, 1])], name="swap")]
    msg = load_error(api, tmp_path, W.model("t", nodes, inits, [W.value_info("X", ["N", 4, 2, 3])], [W.value_info("Y", ["N", 6, 4])], opset=13))
    assert "node 'swap' (Transpose)" in msg and "would need data moved" in msg, msg
    # Flatten(axis = 2) anywhere else keeps its refusal
    nodes = [W.node("Relu", ["X"], ["R"]), W.node("Flatten", ["R"], ["Y"], [W.attr_i("axis", 2)], name="flat2")]
    msg = load_error(api, tmp_path, W.model("f", nodes, [], [W.value_info("X", ["N", 4, 2, 3])], [W.value_info("Y", ["M", 6])], opset=13))
    assert "node 'flat2' (Flatten)" in msg and "only axis=1 keeps the row axis" in msg, msg
    # a Transpose(0,2,1) behind a step that moves nothing (C = 1 or S = 1) was an alias before and is one now, so that these graphs, which
    # loaded before, keep their plans (the kinds below are the parent's) ...
    f32, i64 = lambda nm, v: W.tensor(nm, np.asarray(v, np.float32)), lambda nm, v: W.tensor(nm, np.asarray(v, np.int64))  # noqa: E731
    swap = lambda a, b, nm: W.node("Transpose", [a], [b], [W.attr_ints("perm", [0, 2, 1])], name=nm)  # noqa: E731
    conv1 = lambda a, w, b: W.node("Conv", [a, w], [b], [W.attr_ints("kernel_shape", [3]), W.attr_ints("pads", [1, 1])])  # noqa: E731
    nodes = [conv1("X", "w", "c"), swap("c", "t", "there"), swap("t", "u", "back"), W.node("Relu", ["u"], ["Y"])]
    p = plan_of(api, tmp_path, W.model("c1", nodes, [f32("w", np.ones((1, 3, 3)))], [W.value_info("X", ["N", 3, 8])], [W.value_info("Y", ["N", 1, 8])], opset=13))
    assert kinds(p) == ["Conv2d"] and "tokens" not in p, kinds(p)
    eca = [W.node("Conv", ["X", "w0"], ["f"], [W.attr_ints("kernel_shape", [1, 1])]), W.node("GlobalAveragePool", ["f"], ["g"]), W.node("Reshape", ["g", "s"], ["r"]),
           swap("r", "t", "there"), conv1("t", "w", "c"), swap("c", "u", "back"), W.node("Sigmoid", ["u"], ["Y"])]
    inits = [f32("w0", np.ones((4, 3, 1, 1))), i64("s", [0, 4, 1]), f32("w", np.ones((1, 1, 3)))]
    p = plan_of(api, tmp_path, W.model("eca", eca, inits, [W.value_info("X", ["N", 3, 5, 5])], [W.value_info("Y", ["N", 4, 1])], opset=13))
    assert kinds(p) == ["Conv2d", "GlobalAvgPool", "Conv2d"] and "tokens" not in p, kinds(p)
    nodes = [W.node("Relu", ["X"], ["f"]), W.node("GlobalAveragePool", ["f"], ["g"]), W.node("Reshape", ["g", "s"], ["r"]), swap("r", "t", "there"), W.node("MatMul", ["t", "m"], ["Y"])]
    p = plan_of(api, tmp_path, W.model("gm", nodes, [i64("s", [0, 4, 1]), f32("m", np.ones((4, 2)))], [W.value_info("X", ["N", 4, 5, 5])], [W.value_info("Y", ["N", 1, 2])], opset=13))
    assert kinds(p)[1:] == ["GlobalAvgPool", "Dense"] and "tokens" not in p, kinds(p)
    # ... with no cap on their extents
    nodes = [W.node("Relu", ["X"], ["f"]), swap("f", "Y", "long")]
    p = plan_of(api, tmp_path, W.model("long", nodes, [], [W.value_info("X", ["N", 1, (1 << 20) + 4])], [W.value_info("Y", ["N", (1 << 20) + 4, 1])], opset=13))
    assert kinds(p) == ["Unary"], kinds(p)
    # and only constant rows joined in front make such a value a Tokens step, written by the Concat
    one = plan_of(api, tmp_path, W.tokens_model(1, (4, 5), prefix=0, pos=True)[0])
    assert kinds(one)[0] == "Unary" and "Tokens" not in kinds(one) and "tokens" not in one, kinds(one)  # (the position Add stays the step it was)
    for c, hw in ((1, (4, 5)), (8, (1, 1))):
        s = tokens_step(plan_of(api, tmp_path, W.tokens_model(c, hw, prefix=2, pos=True)[0]))
        assert (s["C"], s["S"], s["prefix"], s["pos"], s["T"], s["E"]) == (c, hw[0] * hw[1], 2, True, 2 + hw[0] * hw[1], c), s
    # models that loaded before have no Tokens step
    for blob in (W.resnet18(classes=10, in_hw=32, width=8), W.transformer_from_spec(W.transformer_spec(T=8, F=4, E=16, h=2, ff=32, layers=1))):
        p = plan_of(api, tmp_path, blob)
        assert "Tokens" not in kinds(p) and "tokens" not in p
