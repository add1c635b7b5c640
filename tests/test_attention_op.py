"""The opset-23 operators Attention and RMSNormalization at load time (no GPU; INTEGRATION.md section 2.6 "The Attention operator",
"RMSNormalization"): every operand form lowers to ONE Attention step with the expected fields and nothing for the Reshape / Transpose / mask
nodes around it, every refusal names its node, and RMSNormalization lowers to ONE RmsNorm step."""
from __future__ import annotations

import os

import numpy as np
import pytest

from infera_amd import onnx_writer as W

NEG_INF = float("-inf")
T, HQ, DH = 8, 4, 4
E = HQ * DH


@pytest.fixture(scope="module")
def api(built):
    from infera_amd import capi

    return capi


def plan_of(api, tmp_path, blob, name="attn_op"):
    path = W.write(os.path.join(str(tmp_path), name + ".onnx"), blob)
    api.load_model(name, path)
    try:
        return api.get_plan(name)["plan"]
    finally:
        api.unload_model(name)


def load_error(api, tmp_path, blob, name="bad"):
    path = W.write(os.path.join(str(tmp_path), name + ".onnx"), blob)
    with pytest.raises(Exception) as e:
        api.load_model(name, path)
        api.unload_model(name)
    return str(e.value)


def kinds(plan):
    return [s["kind"] for s in plan["steps"]]


# ---- Attention: what loads ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["4d", "3d"])
def test_self_attention_is_one_step(api, tmp_path, form):
    p = plan_of(api, tmp_path, W.attention_op_model(T, T, HQ, HQ, DH, form=form))
    assert kinds(p) == ["SliceCols"] * 3 + ["Attention"], kinds(p)  # the Reshape / Transpose around the node emit nothing
    att = p["steps"][-1]
    assert (att["T"], att["heads"], att["dh"], att["mask"], att["packed_qkv"]) == (T, HQ, DH, False, False)
    assert att["scale"] == 0.5 and not ({"Tk", "kv_heads", "causal", "row_mask"} & set(att)), att
    assert att["origin"] == ("Attention:a_attn+...+Reshape:a_merge_heads" if form == "4d" else "Attention:a_attn")
    assert p["output_shape"] == [-1, T, E] and p["flops_per_row"] == 4 * T * T * E


@pytest.mark.parametrize("form", ["4d", "3d"])
def test_packed_projection_is_read_in_place(api, tmp_path, form):
    p = plan_of(api, tmp_path, W.attention_op_model(T, T, HQ, HQ, DH, form=form, packed=True))
    assert kinds(p) == ["Attention"], kinds(p)  # the Split is absorbed: the step reads the packed window with offsets
    assert p["steps"][0]["packed_qkv"] is True


@pytest.mark.parametrize("form", ["4d", "3d"])
def test_causal_grouped_cross(api, tmp_path, form):
    p = plan_of(api, tmp_path, W.attention_op_model(5, 9, 6, 2, 5, form=form, causal=True, scale=0.375))
    att = p["steps"][-1]
    assert (att["T"], att["Tk"], att["heads"], att["kv_heads"], att["dh"], att["causal"], att["scale"]) == (5, 9, 6, 2, 5, True, 0.375), att
    assert p["output_shape"] == [-1, 5, 30] and p["flops_per_row"] == 4 * 5 * 9 * 30
    assert p["input_shape"] == [-1, 5 * 30 + 2 * 9 * 10]


def test_default_scale_is_one_over_sqrt_dh(api, tmp_path):
    att = plan_of(api, tmp_path, W.attention_op_model(T, T, 2, 2, 5))["steps"][-1]
    assert np.float32(att["scale"]) == np.float32(1.0 / np.sqrt(5.0)) or abs(att["scale"] - 1.0 / np.sqrt(5.0)) < 1e-6


@pytest.mark.parametrize("mask,int32_data", [(np.tril(np.ones((T, T), bool)), False), (np.tril(np.ones((T, T), bool)), True), (np.tril(np.ones((1, T, T), bool)), False),
                                             (W.causal_mask(T, 4), False), (W.causal_mask(T, 2), False)], ids=["bool2", "bool2_int32_data", "bool3", "f32_4", "f32_2"])
def test_constant_masks(api, tmp_path, mask, int32_data):
    nodes, inits = [], [W.tensor("a_mask", mask, int32_data=int32_data)]
    for nm in "qkv":
        inits.append(W.tensor(nm + "_shape", np.asarray([-1, T, E], np.int64)))
        nodes.append(W.node("Reshape", [nm.upper(), nm + "_shape"], [nm]))
    out = W.attention_op_nodes(nodes, inits, "a_", "q", "k", "v", T, T, HQ, HQ, DH, form="3d", mask_value="a_mask")
    blob = W.model("m", nodes, inits, [W.value_info(n, ["N", T * E]) for n in "QKV"], [W.value_info(out, ["N", T, E])], opset=23)
    att = plan_of(api, tmp_path, blob)["steps"][-1]
    assert att["mask"] is True and "row_mask" not in att and "causal" not in att


ROW_MASKS = [dict(kind="cast"), dict(kind="cast", lift="reshape"), dict(kind="ids", pad=3), dict(kind="ids", pad=3, lift="reshape")]


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("form", ["4d", "3d"])
@pytest.mark.parametrize("rm", ROW_MASKS, ids=lambda r: "-".join(str(v) for v in r.values()))
def test_row_masks(api, tmp_path, rm, form, causal):
    p = plan_of(api, tmp_path, W.attention_op_model(T, T, HQ, 2, DH, form=form, causal=causal, row_mask=rm))
    assert kinds(p) == ["SliceCols"] * 3 + ["Attention"], kinds(p)  # nothing for the mask sub-graph, no SliceCols of M
    att = p["steps"][-1]
    want = {"src_col": T * E + 2 * T * 2 * DH, "cmp": 3 if rm["kind"] == "ids" else 0, "fill": NEG_INF, "mode": "replace", "excluding": True}
    assert att["row_mask"] == want, att["row_mask"]
    assert att.get("causal", False) is causal and att["mask"] is False and att["kv_heads"] == 2


@pytest.mark.parametrize("mask_type", [W.INT64, W.INT32, W.FLOAT], ids=["int64", "int32", "f32"])
def test_row_mask_input_types(api, tmp_path, mask_type):
    p = plan_of(api, tmp_path, W.attention_op_model(T, T, HQ, HQ, DH, row_mask=dict(kind="cast"), mask_type=mask_type))
    assert p["steps"][-1]["row_mask"]["src_col"] == 3 * T * E


def test_opset_24_loads(api, tmp_path):
    assert kinds(plan_of(api, tmp_path, W.attention_op_model(T, T, HQ, HQ, DH, opset=24)))[-1] == "Attention"


def test_decoder_block_plan(api, tmp_path):
    spec = W.decoder_block_spec()
    for form in ("4d", "3d"):
        p = plan_of(api, tmp_path, W.decoder_block_from_spec(spec, form=form))
        per_layer = ["RmsNorm", "Dense", "Dense", "Dense", "Attention", "Dense", "BinaryAct", "RmsNorm", "Dense", "Dense", "BinaryAct", "Dense", "BinaryAct"]
        assert kinds(p) == per_layer * 2 + ["RmsNorm", "SliceCols", "Dense"], kinds(p)
        att = [s for s in p["steps"] if s["kind"] == "Attention"]
        assert all(s["causal"] is True and s["kv_heads"] == spec["hkv"] and s["heads"] == spec["hq"] and "Tk" not in s for s in att)
        assert [s.get("act") for s in p["steps"] if s["kind"] == "Dense"][4] == "Swish"


# ---- Attention: refusals -------------------------------------------------------------------------------------------------------------------

def by_hand(Eq, Ek, Ev, hq, hkv, Tq=T, Tk=T, **kw):
    """the 3-D form over operands of any widths"""
    nodes, inits = [], []
    for nm, t, e in (("q", Tq, Eq), ("k", Tk, Ek), ("v", Tk, Ev)):
        inits.append(W.tensor(nm + "_shape", np.asarray([-1, t, e], np.int64)))
        nodes.append(W.node("Reshape", [nm.upper(), nm + "_shape"], [nm]))
    out = W.attention_op_nodes(nodes, inits, "a_", "q", "k", "v", Tq, Tk, hq, hkv, 1, form="3d", **kw)
    ins = [W.value_info("Q", ["N", Tq * Eq]), W.value_info("K", ["N", Tk * Ek]), W.value_info("V", ["N", Tk * Ev])]
    return W.model("m", nodes, inits, ins, [W.value_info(out, ["N", Tq, Eq])], opset=23)


def query_dependent_row_mask():
    """a bool mask [N, 1, Tq, Tk] from an input of Tq Tk columns"""
    nodes, inits = [], [W.tensor("s4", np.asarray([-1, 1, T, T], np.int64))]
    for nm in "qkv":
        inits.append(W.tensor(nm + "_shape", np.asarray([-1, T, E], np.int64)))
        nodes.append(W.node("Reshape", [nm.upper(), nm + "_shape"], [nm]))
    nodes += [W.node("Cast", ["M"], ["mb"], [W.attr_i("to", W.BOOL)]), W.node("Reshape", ["mb", "s4"], ["m4"])]
    out = W.attention_op_nodes(nodes, inits, "a_", "q", "k", "v", T, T, HQ, HQ, DH, mask_value="m4")
    ins = [W.value_info(n, ["N", T * E]) for n in "QKV"] + [W.value_info("M", ["N", T * T], W.INT64)]
    return W.model("m", nodes, inits, ins, [W.value_info(out, ["N", T, E])], opset=23)


def head_major_input():
    nodes = [W.node("Attention", ["X", "X", "X"], ["Y"], name="a_attn")]
    return W.model("m", nodes, [], [W.value_info("X", ["N", HQ, T, DH])], [W.value_info("Y", ["N", HQ, T, DH])], opset=23)


def y_served_head_major():
    nodes, inits = [], []
    for nm in "qkv":
        inits.append(W.tensor(nm + "_shape", np.asarray([-1, T, E], np.int64)))
        nodes.append(W.node("Reshape", [nm.upper(), nm + "_shape"], [nm]))
    W.attention_op_nodes(nodes, inits, "a_", "q", "k", "v", T, T, HQ, HQ, DH)
    return W.model("m", nodes, inits, [W.value_info(n, ["N", T * E]) for n in "QKV"], [W.value_info("a_y4", ["N", HQ, T, DH])], opset=23)


def all_inf_row():
    mk = W.causal_mask(T)
    mk[3, :] = -np.inf
    return mk


REFUSALS = {
    "past_key": (lambda: W.attention_op_model(T, T, HQ, HQ, DH, extra_inputs=["pk", "pv"]), "past_key / past_value"),
    "present_key": (lambda: W.attention_op_model(T, T, HQ, HQ, DH, form="3d", extra_outputs=["pk_out"], graph_outputs=["pk_out"]), "output present_key is consumed"),
    "qk_matmul_output": (lambda: W.attention_op_model(T, T, HQ, HQ, DH, form="3d", extra_outputs=["", "", "qk"], graph_outputs=["qk"]), "output qk_matmul_output is consumed"),
    "nonpad_kv_seqlen": (lambda: W.attention_op_model(T, T, HQ, HQ, DH, opset=24, extra_inputs=["", "", "L"]), "nonpad_kv_seqlen"),
    "softcap": (lambda: W.attention_op_model(T, T, HQ, HQ, DH, extra_attrs=[W.attr_f("softcap", 30.0)]), "softcap"),
    "softmax_precision": (lambda: W.attention_op_model(T, T, HQ, HQ, DH, extra_attrs=[W.attr_i("softmax_precision", W.FLOAT16)]), "softmax_precision"),
    "v_head_size": (lambda: by_hand(8, 8, 16, 2, 2), "v_head_size = 8 differs from head_size = 4"),
    "heads_not_grouped": (lambda: W.attention_op_model(T, T, 3, 2, DH, form="3d"), "q_num_heads = 3 is no multiple of kv_num_heads = 2"),
    "heads_not_grouped_4d": (lambda: W.attention_op_model(T, T, 3, 2, DH, form="4d"), "q_num_heads = 3 is no multiple of kv_num_heads = 2"),
    "head_mask": (lambda: W.attention_op_model(T, T, HQ, HQ, DH, mask=np.zeros((HQ, T, T), np.float32)), "depends on the row or the head"),
    "query_row_mask": (query_dependent_row_mask, "depends on the head or the query"),
    "float_row_mask": (lambda: W.attention_op_model(T, T, HQ, HQ, DH, row_mask=dict(kind="float")), "float (or integer) mask that depends on the row"),
    "masked_is_true": (lambda: W.attention_op_model(T, T, HQ, HQ, DH, row_mask=dict(kind="equal", pad=3)), "write Not(Equal"),
    "inf_row": (lambda: W.attention_op_model(T, T, HQ, HQ, DH, mask=all_inf_row()), "row 3 of the attention mask is -inf everywhere"),
    "inf_row_under_causal": (lambda: W.attention_op_model(T, T, HQ, HQ, DH, causal=True, mask=np.triu(np.ones((T, T), bool), 1)), "row 0 of the attention mask is -inf everywhere"),
    "nan_mask": (lambda: W.attention_op_model(T, T, HQ, HQ, DH, mask=np.full((T, T), np.nan, np.float32)), "NaN or +inf"),
    "plus_inf_mask": (lambda: W.attention_op_model(T, T, HQ, HQ, DH, mask=np.full((T, T), np.inf, np.float32)), "NaN or +inf"),
    "mask_shape": (lambda: W.attention_op_model(T, T, HQ, HQ, DH, mask=np.zeros((T, T + 1), np.float32)), "does not broadcast"),
    "Tq_cap": (lambda: W.attention_op_model(1025, 8, 1, 1, 4), "T = 1025 is beyond"),
    "Tk_cap": (lambda: W.attention_op_model(8, 1025, 1, 1, 4), "Tk = 1025 is beyond"),
    "dh_cap": (lambda: W.attention_op_model(T, T, 1, 1, 129), "dh = 129 is beyond"),
    "heads_cap": (lambda: W.attention_op_model(2, 2, 1025, 1025, 1), "h = 1025 is beyond"),
    "scale": (lambda: W.attention_op_model(T, T, HQ, HQ, DH, scale=-1.0), "scale must be a positive finite"),
    "head_major_input": (head_major_input, "a head-major [N,h,T,dh] tensor"),
    "y_head_major": (y_served_head_major, "Y is read as [N,h,T,dh] by the graph output"),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refusals_name_their_node(api, tmp_path, case):
    build, why = REFUSALS[case]
    msg = load_error(api, tmp_path, build())
    assert "node 'a_attn' (Attention): unsupported operator form: " in msg and why in msg, msg


# ---- RMSNormalization ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T_", [0, 3])
def test_rmsnorm_is_one_step(api, tmp_path, T_):
    p = plan_of(api, tmp_path, W.rmsnorm_model(33, 1e-6, np.ones(33), T=T_))
    assert kinds(p) == ["RmsNorm"]
    s = p["steps"][0]
    assert (s["E"], s["T"], s["origin"]) == (33, max(T_, 1), "RMSNormalization:rms") and abs(s["eps"] - 1e-6) < 1e-12
    assert p["output_shape"] == ([-1, T_, 33] if T_ else [-1, 33])


RMS_REFUSALS = {
    "axis": (lambda: W.rmsnorm_model(8, 1e-5, np.ones(8), T=3, axis=1), "only normalisation over the last axis"),
    "scale_not_constant": (lambda: W.rmsnorm_model(8, 1e-5, None, scale_input=True), "scale is not a constant"),
    "scale_length": (lambda: W.rmsnorm_model(8, 1e-5, np.ones(9)), "scale must be a vector of E = 8 elements"),
    "scale_rank": (lambda: W.rmsnorm_model(8, 1e-5, np.ones((1, 8))), "scale must be a vector of E = 8 elements"),
    "cap": (lambda: W.rmsnorm_model(4097, 1e-5, np.ones(4097)), "E = 4097 is beyond the RmsNorm kernel's cap"),
    "stash_type": (lambda: W.rmsnorm_model(8, 1e-5, np.ones(8), extra_attrs=[W.attr_i("stash_type", W.FLOAT16)]), "stash_type"),
    "epsilon": (lambda: W.rmsnorm_model(8, -1.0, np.ones(8)), "epsilon must be a finite number >= 0"),
}


@pytest.mark.parametrize("case", sorted(RMS_REFUSALS))
def test_rmsnorm_refusals_name_their_node(api, tmp_path, case):
    build, why = RMS_REFUSALS[case]
    msg = load_error(api, tmp_path, build())
    assert "node 'rms' (RMSNormalization): unsupported operator form: " in msg and why in msg, msg


def test_bool_tensors_keep_the_size_checks(api, tmp_path):
    """a BOOL initializer whose payload is shorter than its dims is refused by the parser, in raw_data and in int32_data"""
    for int32_data in (False, True):
        good = W.tensor("a_mask", np.ones((T, T), bool), int32_data=int32_data)
        short = W.tensor("a_mask", np.ones((T, T - 1), bool), int32_data=int32_data)
        dims_of_good = b"".join(W._vi(1, d) for d in (T, T))
        bad = dims_of_good + short[len(b"".join(W._vi(1, d) for d in (T, T - 1))):]
        assert good.startswith(dims_of_good)
        nodes, inits = [], [bad]
        for nm in "qkv":
            inits.append(W.tensor(nm + "_shape", np.asarray([-1, T, E], np.int64)))
            nodes.append(W.node("Reshape", [nm.upper(), nm + "_shape"], [nm]))
        out = W.attention_op_nodes(nodes, inits, "a_", "q", "k", "v", T, T, HQ, HQ, DH, form="3d", mask_value="a_mask")
        blob = W.model("m", nodes, inits, [W.value_info(n, ["N", T * E]) for n in "QKV"], [W.value_info(out, ["N", T, E])], opset=23)
        assert "element count does not match dims" in load_error(api, tmp_path, blob)
