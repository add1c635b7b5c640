"""Transformer encoders at load time (no GPU): the plan a model lowers to (window Dense, merged QKV projection, Attention, LayerNorm, mean over
time), the equivalence of the exporter spellings, flops_per_row, and the rejections of INTEGRATION.md section 2.6."""
from __future__ import annotations

import os

import numpy as np
import pytest

from infera_amd import onnx_writer as W


@pytest.fixture(scope="module")
def api(built):
    from infera_amd import capi

    return capi


def plan_of(api, tmp_path, blob, name="tfm", select=""):
    path = W.write(os.path.join(str(tmp_path), name + ".onnx"), blob)
    api.load_model(name, path + select)
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
    """The steps without origins, buffers renumbered in order of first appearance (a merged projection leaves unused buffer ids behind)."""
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


SPEC = dict(T=24, F=8, E=64, h=4, ff=256, layers=2)


def test_two_layer_encoder_plan(api, tmp_path):
    spec = W.transformer_spec(**SPEC)
    p = plan_of(api, tmp_path, W.transformer_from_spec(spec))
    layer = ["Dense", "Attention", "Dense", "BinaryAct", "LayerNorm", "Dense", "Dense", "BinaryAct", "LayerNorm"]
    assert kinds(p) == ["Dense", "BinaryConst"] + layer * 2 + ["MeanTime", "Dense"], kinds(p)
    st = p["plan"]["steps"]
    assert "ChannelShuffle" not in kinds(p) and "Softmax" not in kinds(p)
    assert (st[0]["K"], st[0]["M"], st[0]["T"]) == (8, 64, 24)  # the input projection is a window Dense
    qkv, att = st[2], st[3]
    assert (qkv["K"], qkv["M"], qkv["T"], qkv["bias"]) == (64, 192, 24, True)  # Q, K, V merged: the value is read once
    assert att["packed_qkv"] and att["in"] == att["in1"] == att["in2"] == qkv["out"]
    assert (att["T"], att["heads"], att["dh"], att["mask"]) == (24, 4, 16, False) and att["scale"] == pytest.approx(0.25)
    assert (st[7]["M"], st[7]["act"], st[8]["M"]) == (256, "Relu", 64)  # the feed-forward pair, activation fused
    assert st[6]["E"] == 64 and st[6]["T"] == 24
    assert p["plan"]["output_shape"] == [-1, 1]
    # 2 T K M per window Dense, 4 T^2 E per attention step, 2 K M for the head
    T, F, E, ff = 24, 8, 64, 256
    per_layer = 2 * T * E * 3 * E + 4 * T * T * E + 2 * T * E * E + 2 * T * E * ff + 2 * T * ff * E
    assert p["plan"]["flops_per_row"] == 2 * T * F * E + 2 * per_layer + 2 * E * 1


@pytest.mark.parametrize("kw", [dict(qkv="packed_split"), dict(qkv="packed_slice"), dict(scale="scores_mul"), dict(scale="q"), dict(scale="sqrt_both"),
                                dict(k_transpose="two_step"), dict(shape="subgraph"), dict(shape="subgraph", qkv="packed_split", scale="sqrt_both")],
                         ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
@pytest.mark.parametrize("causal", [False, True])
def test_spellings_give_one_plan(api, tmp_path, kw, causal):
    spec = W.transformer_spec(causal=causal, **SPEC)
    plain = plan_of(api, tmp_path, W.transformer_from_spec(spec), "plain")
    other = plan_of(api, tmp_path, W.transformer_from_spec(spec, **kw), "other")
    assert canon(other) == canon(plain)
    assert [s["mask"] for s in plain["plan"]["steps"] if s["kind"] == "Attention"] == [causal, causal]


def test_mask_forms_and_prenorm_gelu_heads(api, tmp_path):
    spec = W.transformer_spec(causal=True, norm_first=True, act="Gelu", **SPEC)
    a = plan_of(api, tmp_path, W.transformer_from_spec(spec, mask_rank=2), "m2")
    b = plan_of(api, tmp_path, W.transformer_from_spec(spec, mask_rank=4), "m4")
    assert canon(a) == canon(b)
    assert kinds(a).count("LayerNorm") == 5 and kinds(a).count("Attention") == 2
    blob = W.transformer_from_spec(spec, heads=("mean", "first", "last", "seq"))
    assert plan_of(api, tmp_path, blob, "h0")["plan"]["output_shape"] == [-1, 1]
    assert kinds(plan_of(api, tmp_path, blob, "h1", "#first"))[-2:] == ["SliceCols", "Dense"]
    assert kinds(plan_of(api, tmp_path, blob, "h2", "#last"))[-2:] == ["SliceCols", "Dense"]
    seq = plan_of(api, tmp_path, blob, "h3", "#seq")
    assert seq["plan"]["output_shape"] == [-1, 24, 1] and seq["plan"]["steps"][-1]["T"] == 24
    keep = plan_of(api, tmp_path, W.transformer_from_spec(spec, keepdims=1), "kd")
    assert keep["plan"]["output_shape"] == [-1, 1, 1]


def test_rank3_glue_plans(api, tmp_path):
    """Positional [1,T,E] constant -> BinaryConst over T*E; residual Add -> BinaryAct; the decomposed GELU stays five elementwise steps."""
    spec = W.transformer_spec(act="Gelu", T=6, F=4, E=8, h=2, ff=16, layers=1)
    op = plan_of(api, tmp_path, W.transformer_from_spec(spec), "g_op")
    dec = plan_of(api, tmp_path, W.transformer_from_spec(spec, gelu="decomposed"), "g_dec")
    assert len(kinds(dec)) > len(kinds(op)) and kinds(dec).count("Attention") == 1  # (not fused in this change: separate elementwise passes)
    assert any(s.get("act") == "Gelu" for s in op["plan"]["steps"])
    assert kinds(op)[1] == "BinaryConst"


def test_lstm_then_per_step_linear_loads(api, tmp_path):
    spec = W.recurrent_spec("LSTM", T=10, F=4, H=16)
    base = W.recurrent_from_spec(spec, form="layout1", tail="seq", flat=True)
    # append MatMul [16, 3] + Add to Y [N, T, 16]: rebuilt through the writer's primitives
    rng = np.random.default_rng(0)
    Wd, bd = rng.standard_normal((16, 3)).astype(np.float32), rng.standard_normal(3).astype(np.float32)
    blob = lstm_linear(spec, Wd, bd)
    p = plan_of(api, tmp_path, blob, "lstm_lin")
    assert kinds(p) == ["Recurrent", "Dense"] and p["plan"]["steps"][1]["T"] == 10 and p["plan"]["output_shape"] == [-1, 10, 3]
    assert plan_of(api, tmp_path, base, "lstm_base")["plan"]["output_shape"] == [-1, 10, 16]


def lstm_linear(spec, Wd, bd):
    T, F, H = spec["T"], spec["F"], spec["H"]
    L = spec["layers"][0]
    inits = [W.tensor("W", L["W"]), W.tensor("R", L["R"]), W.tensor("B", L["B"]), W.tensor("fs", np.asarray([-1, T, F], dtype=np.int64)),
             W.tensor("mg", np.asarray([0, 0, -1], dtype=np.int64)), W.tensor("Wd", Wd), W.tensor("bd", bd)]
    nodes = [W.node("Reshape", ["X", "fs"], ["X3"]),
             W.node("LSTM", ["X3", "W", "R", "B"], ["Y"], [W.attr_i("hidden_size", H), W.attr_i("layout", 1)], name="rnn"),
             W.node("Reshape", ["Y", "mg"], ["S"]), W.node("MatMul", ["S", "Wd"], ["mm"], name="step_linear"), W.node("Add", ["mm", "bd"], ["out"])]
    return W.model("lstm_linear", nodes, inits, [W.value_info("X", ["N", T * F])], [W.value_info("out", ["N", T, 3])], opset=14)


# ---- rejections: node '<name>' (<Op>): unsupported operator form: <why> -----------------------------------------------------------------------

def att(T=8, E=16, h=4, **kw):
    return W.attention_only(T, E, h, form="three", **kw)


def test_rejections_name_the_node_and_the_reason(api, tmp_path):
    err = lambda blob: load_error(api, tmp_path, blob)  # noqa: E731
    e = err(att(softmax_axis=2))
    assert "node 'a_qk' (MatMul)" in e and "unsupported operator form" in e and "Softmax over axis 2" in e
    e = err(att(E=18))  # 18 = 4 * 4 + 2
    assert "node 'a_qk' (MatMul)" in e and "not divisible by h = 4" in e
    full = np.zeros((8, 8), np.float32)
    full[3, :] = -np.inf
    e = err(att(mask=full))
    assert "row 3 of the attention mask is -inf everywhere" in e
    e = err(att(mask=np.zeros((2, 4, 8, 8), np.float32)))
    assert "does not broadcast to [T, T]" in e
    e = err(att(scale_value=-1.0))
    assert "positive finite" in e
    e = err(att(T=2048, E=8, h=2))
    assert "beyond the attention kernel's cap of 1024 steps" in e
    e = err(att(T=4, E=512, h=2))
    assert "dh = 256 is beyond the attention kernel's cap of 128" in e


def graph(nodes, inits, in_dims, out_dims, opset=20, ins=None):
    return W.model("g", nodes, inits, ins or [W.value_info("X", in_dims)], [W.value_info("out", out_dims)], opset=opset)


def i64(name, v):
    return W.tensor(name, np.asarray(v, dtype=np.int64))


def f32(name, v):
    return W.tensor(name, np.asarray(v, dtype=np.float32))


def test_rejected_graph_forms(api, tmp_path):
    err = lambda blob: load_error(api, tmp_path, blob)  # noqa: E731
    # MatMul of two activations with no attention pattern around it
    e = err(graph([W.node("Reshape", ["X", "s"], ["a"]), W.node("MatMul", ["a", "a"], ["out"], name="gram")], [i64("s", [-1, 4, 4])], ["N", 16], ["N", 4, 4]))
    assert "node 'gram' (MatMul)" in e and "unsupported operator form" in e and "outside a recognised self-attention pattern" in e
    # a mask computed from the row
    e = err(row_mask_graph())
    assert "is not a constant" in e and "node 'a_qk' (MatMul)" in e
    # cross-attention: K and V over another window length
    e = err(cross_attention_graph())
    assert "different window lengths T" in e and "cross-attention is not supported" in e
    # LayerNormalization forms
    ln = lambda attrs, outs=("out",), extra=(): graph([W.node("Reshape", ["X", "s"], ["a"]), W.node("LayerNormalization", ["a", "g", "b"], list(outs), attrs, name="ln")] + list(extra),  # noqa: E731
                                                      [i64("s", [-1, 4, 8]), f32("g", np.ones(8)), f32("b", np.zeros(8))], ["N", 32], ["N", 4, 8])
    e = err(ln([W.attr_i("axis", 1)]))
    assert "node 'ln' (LayerNormalization)" in e and "only normalisation over the last axis" in e
    e = err(graph([W.node("Reshape", ["X", "s"], ["a"]), W.node("LayerNormalization", ["a", "g", "b"], ["y", "mean"], [W.attr_i("axis", -1)], name="ln"),
                   W.node("Add", ["y", "mean"], ["out"])], [i64("s", [-1, 4, 8]), f32("g", np.ones(8)), f32("b", np.zeros(8))], ["N", 32], ["N", 4, 8]))
    assert "output Mean is consumed" in e
    # contrib fused operators
    for op in ("Attention", "MultiHeadAttention", "SkipLayerNormalization"):
        e = err(graph([W.node(op, ["X", "g", "b"], ["out"], name="fused", domain="com.microsoft")], [f32("g", np.ones(8)), f32("b", np.zeros(8))], ["N", 8], ["N", 8]))
        assert f"node 'fused' ({op})" in e and "contrib fused operator" in e
    # symbolic T
    e = err(graph([W.node("Identity", ["X"], ["out"])], [], ["N", "T", 8], ["N", "T", 8]))
    assert "only the leading (row/batch) dimension of the input may be symbolic" in e


def row_mask_graph():
    nodes, inits = [], [i64("x_shape", [-1, 8, 48]), i64("sp", [16, 16, 16]), i64("ms", [-1, 1, 8, 8]), i64("m_b", [0]), i64("m_e", [64]), i64("ax1", [1])]
    nodes += [W.node("Reshape", ["X", "x_shape"], ["X3"]), W.node("Split", ["X3", "sp"], ["q", "k", "v"], [W.attr_i("axis", 2)]),
              W.node("Slice", ["X", "m_b", "m_e", "ax1"], ["mflat"]), W.node("Reshape", ["mflat", "ms"], ["rowmask"])]
    p, T, E, h, dh = "a_", 8, 16, 4, 4
    inits += [i64(p + "split", [0, T, h, dh]), i64(p + "merge", [0, T, E])]
    for nm in "qkv":
        nodes.append(W.node("Reshape", [nm, p + "split"], [p + nm + "4"]))
        nodes.append(W.node("Transpose", [p + nm + "4"], [p + nm + "h"], [W.attr_ints("perm", [0, 2, 3, 1] if nm == "k" else [0, 2, 1, 3])]))
    nodes += [W.node("MatMul", [p + "qh", p + "kh"], [p + "s0"], name=p + "qk"), W.node("Add", [p + "s0", "rowmask"], [p + "s1"]),
              W.node("Softmax", [p + "s1"], [p + "p"], [W.attr_i("axis", -1)]), W.node("MatMul", [p + "p", p + "vh"], [p + "o4"]),
              W.node("Transpose", [p + "o4"], [p + "ot"], [W.attr_ints("perm", [0, 2, 1, 3])]), W.node("Reshape", [p + "ot", p + "merge"], ["out"])]
    return graph(nodes, inits, ["N", 8 * 48], ["N", 8, 16])


def cross_attention_graph():
    # Q over 8 steps, K / V over 4: two inputs
    inits = [i64("qs", [-1, 8, 16]), i64("ks", [-1, 4, 32]), i64("sp", [16, 16]), i64("q4", [0, 8, 4, 4]), i64("k4", [0, 4, 4, 4]), i64("merge", [0, 8, 16])]
    nodes = [W.node("Reshape", ["Q", "qs"], ["q"]), W.node("Reshape", ["KV", "ks"], ["kv"]), W.node("Split", ["kv", "sp"], ["k", "v"], [W.attr_i("axis", 2)]),
             W.node("Reshape", ["q", "q4"], ["q_4"]), W.node("Reshape", ["k", "k4"], ["k_4"]), W.node("Reshape", ["v", "k4"], ["v_4"]),
             W.node("Transpose", ["q_4"], ["qh"], [W.attr_ints("perm", [0, 2, 1, 3])]), W.node("Transpose", ["k_4"], ["kh"], [W.attr_ints("perm", [0, 2, 3, 1])]),
             W.node("Transpose", ["v_4"], ["vh"], [W.attr_ints("perm", [0, 2, 1, 3])]), W.node("MatMul", ["qh", "kh"], ["s"], name="a_qk"),
             W.node("Softmax", ["s"], ["p"], [W.attr_i("axis", -1)]), W.node("MatMul", ["p", "vh"], ["o4"]),
             W.node("Transpose", ["o4"], ["ot"], [W.attr_ints("perm", [0, 2, 1, 3])]), W.node("Reshape", ["ot", "merge"], ["out"])]
    return graph(nodes, inits, None, ["N", 8, 16], ins=[W.value_info("Q", ["N", 128]), W.value_info("KV", ["N", 128])])


@pytest.mark.parametrize("T,E,h", [(3, 16, 4), (-3, 16, 4), (8, 0, 4), (8, 16, 0), (8, 16, -2), (8, 16, 5), (2 ** 40, 16, 4), (8, 2 ** 40, 4), (8, 16, 2 ** 40)])
def test_hostile_shapes_fail_cleanly(api, tmp_path, T, E, h):
    """The head-split target is taken from the file (0 = copy, as ONNX reads it): wrong / zero / negative / overflowing extents and h not dividing E are load errors, not crashes."""
    inits = [i64("x_shape", [-1, 8, 48]), i64("sp", [16, 16, 16]), i64("a_split", [0, T, h, E // h if h > 0 else 0]), i64("a_merge", [0, 8, 16])]
    nodes = [W.node("Reshape", ["X", "x_shape"], ["X3"]), W.node("Split", ["X3", "sp"], ["q", "k", "v"], [W.attr_i("axis", 2)])]
    for nm in "qkv":
        nodes.append(W.node("Reshape", [nm, "a_split"], [nm + "4"]))
        nodes.append(W.node("Transpose", [nm + "4"], [nm + "h"], [W.attr_ints("perm", [0, 2, 3, 1] if nm == "k" else [0, 2, 1, 3])]))
    nodes += [W.node("MatMul", ["qh", "kh"], ["s"], name="a_qk"), W.node("Softmax", ["s"], ["p"], [W.attr_i("axis", -1)]), W.node("MatMul", ["p", "vh"], ["o4"]),
              W.node("Transpose", ["o4"], ["ot"], [W.attr_ints("perm", [0, 2, 1, 3])]), W.node("Reshape", ["ot", "a_merge"], ["out"])]
    e = load_error(api, tmp_path, graph(nodes, inits, ["N", 8 * 48], ["N", 8, 16]))
    assert "node 'a_qk' (MatMul)" in e and "unsupported operator form" in e


# ---- shared projections, decomposed LayerNorm, the remaining rejections -------------------------------------------------------------------

def shared_projection_graph(T=8, K=6, E=16, h=4, seed=0):
    """Two attention blocks (one unmasked, one causal) over the SAME three projections; output = their sum."""
    rng = np.random.default_rng(seed)
    nodes, inits = [W.node("Reshape", ["X", "xs"], ["x3"])], [i64("xs", [-1, T, K])]
    for c in "qkv":
        inits += [f32("W" + c, rng.uniform(-1, 1, (K, E)) / np.sqrt(K)), f32("b" + c, rng.uniform(-1, 1, E))]
        nodes += [W.node("MatMul", ["x3", "W" + c], [c + "_mm"], name=c + "_proj"), W.node("Add", [c + "_mm", "b" + c], [c])]
    a = W.attention_nodes(nodes, inits, "a_", "q", "k", "v", "x3", T, E, h)
    b = W.attention_nodes(nodes, inits, "b_", "q", "k", "v", "x3", T, E, h, mask=W.causal_mask(T))
    nodes.append(W.node("Add", [a, b], ["out"], name="sum"))
    weights = {n: np.frombuffer(b"", np.float32) for n in ()}
    del weights
    return W.model("shared", nodes, inits, [W.value_info("X", ["N", T * K])], [W.value_info("out", ["N", T, E])], opset=20), rng


def test_shared_projections_are_not_merged(api, tmp_path):
    blob, _ = shared_projection_graph()
    p = plan_of(api, tmp_path, blob, "shared")
    st = p["plan"]["steps"]
    assert kinds(p) == ["Dense", "Dense", "Dense", "Attention", "Attention", "BinaryAct"], kinds(p)
    assert [s["M"] for s in st[:3]] == [16, 16, 16]
    for a in st[3:5]:  # both blocks read the three projection buffers as they are
        assert not a["packed_qkv"] and (a["in"], a["in1"], a["in2"]) == (st[0]["out"], st[1]["out"], st[2]["out"])
    assert [a["mask"] for a in st[3:5]] == [False, True]


def ln_graph(E, rank3, form, beta=True):
    rng = np.random.default_rng(E)
    g, b = rng.normal(1, 0.2, E).astype(np.float32), rng.normal(0, 0.2, E).astype(np.float32)
    T = 5 if rank3 else 1
    nodes, inits = [], []
    x = "X"
    if rank3:
        inits.append(i64("s", [-1, T, E]))
        nodes.append(W.node("Reshape", ["X", "s"], ["x3"]))
        x = "x3"
    W.layernorm_nodes(nodes, inits, x, g, b if beta else None, "out", "ln", 1e-5, form)
    return W.model("ln", nodes, inits, [W.value_info("X", ["N", T * E])], [W.value_info("out", ["N", T, E] if rank3 else ["N", E])], opset=20), g, (b if beta else None)


@pytest.mark.parametrize("form", ["decomposed", "decomposed_mul"])
@pytest.mark.parametrize("beta", [True, False])
def test_decomposed_layernorm_rank2_is_the_operators_plan(api, tmp_path, form, beta):
    op = plan_of(api, tmp_path, ln_graph(20, False, "op", beta)[0], "ln_op")
    dec = plan_of(api, tmp_path, ln_graph(20, False, form, beta)[0], "ln_dec")
    assert canon(dec) == canon(op) and kinds(op) == ["LayerNorm"]
    assert op["plan"]["steps"][0]["bias"] == beta


def test_decomposed_layernorm_rank3_keeps_its_existing_plan(api, tmp_path):
    """On [N, T, E] the decomposed form loaded before this change (pooling + per-channel gate steps): that plan is left alone."""
    p = plan_of(api, tmp_path, ln_graph(8, True, "decomposed")[0], "ln3")
    assert "LayerNorm" not in kinds(p) and kinds(p)[0] == "GlobalAvgPool" and len(kinds(p)) >= 6, kinds(p)


def qkv_graph(mutate):
    """attention over three inputs Q, K, V [N, 8*16], with `mutate(nodes, inits)` editing the node list before it is written"""
    T, E, h = 8, 16, 4
    inits = [i64("x_shape", [-1, T, E])]
    nodes = [W.node("Reshape", [nm.upper(), "x_shape"], [nm]) for nm in "qkv"]
    W.attention_nodes(nodes, inits, "a_", "q", "k", "v", "q", T, E, h, mask=np.zeros((T, T), np.float32))
    out = mutate(nodes, inits) or "a_o"
    return W.model("g", nodes, inits, [W.value_info(nm, ["N", T * E]) for nm in "QKV"], [W.value_info(out, ["N", T, E])], opset=20)


def test_more_rejections(api, tmp_path):
    err = lambda blob: load_error(api, tmp_path, blob)  # noqa: E731

    # PyTorch nn.MultiheadAttention's time-major export: [T, N, E] -> Reshape [T, N*h, dh] -> Transpose(1,0,2); K with Transpose(1,2,0)
    def mha():
        T, E, h, dh = 8, 16, 4, 4
        inits = [i64("xs", [-1, T, E]), i64("fold", [T, -1, dh]), i64("back", [T, -1, E])]
        nodes = []
        for nm in "qkv":
            nodes += [W.node("Reshape", [nm.upper(), "xs"], [nm]), W.node("Transpose", [nm], [nm + "t"], [W.attr_ints("perm", [1, 0, 2])]),
                      W.node("Reshape", [nm + "t", "fold"], [nm + "f"]),
                      W.node("Transpose", [nm + "f"], [nm + "h"], [W.attr_ints("perm", [1, 2, 0] if nm == "k" else [1, 0, 2])])]
        nodes += [W.node("MatMul", ["qh", "kh"], ["s"], name="mha_qk"), W.node("Softmax", ["s"], ["p"], [W.attr_i("axis", -1)]), W.node("MatMul", ["p", "vh"], ["o"]),
                  W.node("Transpose", ["o"], ["ot"], [W.attr_ints("perm", [1, 0, 2])]), W.node("Reshape", ["ot", "back"], ["out_t"]),
                  W.node("Transpose", ["out_t"], ["out"], [W.attr_ints("perm", [1, 0, 2])])]
        return W.model("g", nodes, inits, [W.value_info(nm, ["N", T * E]) for nm in "QKV"], [W.value_info("out", ["N", T, E])], opset=20)

    e = err(mha())
    assert "node 'mha_qk' (MatMul)" in e and "unsupported operator form" in e and "time-major export" in e and "not supported yet" in e

    # the packed head split [N,T,3,h,dh] -> Transpose(2,0,3,1,4) -> Gather / Split of the leading 3
    def packed5():
        T, E, h, dh = 8, 16, 4, 4
        inits = [i64("xs", [-1, T, 3, h, dh]), i64("merge", [0, T, E]), i64("ax0", [0])] + [i64("i%d" % j, j) for j in range(3)]
        nodes = [W.node("Reshape", ["X", "xs"], ["x5"]), W.node("Transpose", ["x5"], ["x5t"], [W.attr_ints("perm", [2, 0, 3, 1, 4])])]
        for j, nm in enumerate("qkv"):
            nodes.append(W.node("Gather", ["x5t", "i%d" % j], [nm + "h"], [W.attr_i("axis", 0)]))
        nodes += [W.node("Transpose", ["kh"], ["kt"], [W.attr_ints("perm", [0, 1, 3, 2])]), W.node("MatMul", ["qh", "kt"], ["s"], name="p5_qk"),
                  W.node("Softmax", ["s"], ["p"], [W.attr_i("axis", -1)]), W.node("MatMul", ["p", "vh"], ["o"]),
                  W.node("Transpose", ["o"], ["ot"], [W.attr_ints("perm", [0, 2, 1, 3])]), W.node("Reshape", ["ot", "merge"], ["out"])]
        return W.model("g", nodes, inits, [W.value_info("X", ["N", T * 3 * E])], [W.value_info("out", ["N", T, E])], opset=20)

    e = err(packed5())
    assert "node 'p5_qk' (MatMul)" in e and "Transpose(2,0,3,1,4)" in e and "not supported yet" in e

    # a second mask
    def second_mask(nodes, inits):
        inits.append(f32("mask2", np.zeros((8, 8))))
        i = next(k for k, n in enumerate(nodes) if b"a_softmax" in n)
        nodes[i] = W.node("Softmax", ["a_s3"], ["a_p"], [W.attr_i("axis", -1)], name="a_softmax")
        nodes.insert(i, W.node("Add", ["a_s2", "mask2"], ["a_s3"], name="mask_again"))

    e = err(qkv_graph(second_mask))
    assert "node 'a_qk' (MatMul)" in e and "more than one mask" in e

    # a scale computed from the rows
    def row_scale(nodes, inits):
        inits += [i64("ax12", [1, 2]), i64("u", [0, 1, 1, 1])]
        i = next(k for k, n in enumerate(nodes) if b"a_scale" in n)
        nodes[i] = W.node("Div", ["a_s0", "rs4"], ["a_s1"], name="a_scale")
        nodes.insert(i, W.node("Reshape", ["rs", "u"], ["rs4"]))
        nodes.insert(i, W.node("ReduceMean", ["q", "ax12"], ["rs"], [W.attr_i("keepdims", 0)]))

    e = err(qkv_graph(row_scale))
    assert "node 'a_qk' (MatMul)" in e and "unsupported operator form" in e and "the scale 'rs4' of the attention scores is not a constant" in e

    # caps: heads, LayerNormalization's E
    e = err(W.attention_only(2, 2048, 2048, form="three"))
    assert "h = 2048 is beyond the attention kernel's cap of 1024 heads" in e
    e = err(ln_graph(4100, False, "op")[0])
    assert "node 'ln' (LayerNormalization)" in e and "E = 4100 is beyond the LayerNorm kernel's cap of 4096" in e


def test_rank3_glue_forms(api, tmp_path):
    """[E] scale and bias, a [T, E] positional constant and a residual Add on a window: which steps they become."""
    T, E = 6, 8
    rng = np.random.default_rng(1)
    inits = [i64("s", [-1, T, E]), f32("sc", rng.normal(1, 0.1, E)), f32("bi", rng.normal(0, 0.1, E)), f32("pos", rng.normal(0, 1, (T, E))), f32("half", np.full(E, 0.5))]
    nodes = [W.node("Reshape", ["X", "s"], ["x3"]), W.node("Mul", ["x3", "sc"], ["a"], name="scale_E"), W.node("Add", ["a", "bi"], ["b"], name="bias_E"),
             W.node("Add", ["b", "pos"], ["c"], name="pos_TE"), W.node("Mul", ["c", "half"], ["d"], name="uniform_E"), W.node("Add", ["d", "x3"], ["out"], name="residual")]
    p = plan_of(api, tmp_path, W.model("glue", nodes, inits, [W.value_info("X", ["N", T * E])], [W.value_info("out", ["N", T, E])], opset=20), "glue")
    assert kinds(p) == ["BinaryConst", "BinaryConst", "BinaryConst", "AffineChannel", "BinaryAct"], kinds(p)
    # pos as [T, E] and as [1, T, E]: one plan
    spec = W.transformer_spec(T=6, F=4, E=8, h=2, ff=16, layers=1)
    assert canon(plan_of(api, tmp_path, W.transformer_from_spec(spec, pos_rank=2), "p2")) == canon(plan_of(api, tmp_path, W.transformer_from_spec(spec), "p3"))


def test_conv1d_behind_a_window_step_still_loads(api, tmp_path):
    """LSTM Y [N, T, H] -> Relu -> Conv1d over it as [N, C = T, L = H]: the elementwise value now lies in a flat buffer; the plan's steps are
    what they were."""
    spec = W.recurrent_spec("LSTM", T=6, F=4, H=8)
    L = spec["layers"][0]
    rng = np.random.default_rng(2)
    inits = [W.tensor("W", L["W"]), W.tensor("R", L["R"]), W.tensor("B", L["B"]), i64("fs", [-1, 6, 4]), i64("mg", [0, 0, -1]), f32("cw", rng.normal(0, 0.3, (5, 6, 3)))]
    nodes = [W.node("Reshape", ["X", "fs"], ["X3"]), W.node("LSTM", ["X3", "W", "R", "B"], ["Y"], [W.attr_i("hidden_size", 8), W.attr_i("layout", 1)], name="rnn"),
             W.node("Reshape", ["Y", "mg"], ["S"]), W.node("Relu", ["S"], ["A"]), W.node("Conv", ["A", "cw"], ["out"], [W.attr_ints("kernel_shape", [3])], name="conv1d")]
    p = plan_of(api, tmp_path, W.model("c", nodes, inits, [W.value_info("X", ["N", 24])], [W.value_info("out", ["N", 5, 6])], opset=14), "c1d")
    assert kinds(p) == ["Recurrent", "Unary", "Conv2d"], kinds(p)
    assert p["activation_layout"] == "NCHW"
