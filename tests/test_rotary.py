"""Rotary position embeddings at load time (no GPU; INTEGRATION.md section 2.6 "Rotary position embeddings"): the RotaryEmbedding operator in
its 3-D and 4-D forms and the rotate_half spelling (two Slices or one Split) each lower to ONE Rotary step per rotated operand in front of ONE
Attention step, in front of the Attention operator and of the MatMul / Softmax pattern; a packed projection is still read in place; both
spellings give one plan; every refusal names its node; a sub-graph that is not exactly the spelling is refused as before; and with default
arguments the writers emit the bytes they emitted before the rotary= keyword."""
from __future__ import annotations

import hashlib
import os

import numpy as np
import pytest

from infera_amd import onnx_writer as W

T, HQ, HKV, DH = 8, 4, 2, 8


@pytest.fixture(scope="module")
def api(built):
    from infera_amd import capi

    return capi


def plan_of(api, tmp_path, blob, name="rotary"):
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


def rotary_steps(plan):
    return [s for s in plan["steps"] if s["kind"] == "Rotary"]


def without(step, *keys):
    return {k: v for k, v in step.items() if k not in keys}


# ---- what loads ----------------------------------------------------------------------------------------------------------------------------

def test_the_3d_operator_is_one_window_step(api, tmp_path):
    p = plan_of(api, tmp_path, W.rotary_model(5, 3, 6, rotary={"rd": 4, "interleaved": True}))
    assert kinds(p) == ["Rotary"], kinds(p)
    s = p["steps"][0]
    assert (s["T"], s["heads"], s["dh"], s["rd"], s["interleaved"], s["positions"], s["origin"]) == (5, 3, 6, 4, True, "arange", "RotaryEmbedding:r_rope")
    assert (s["ld"], s["off"], s["form"]) == (18, 0, "scalar")
    assert p["output_shape"] == [-1, 5, 18] and p["flops_per_row"] == 3 * 5 * 3 * 4  # 3 per rotated column
    # any window reader may follow: here, a window Dense behind it
    nodes, inits = [W.node("Reshape", ["X", "s"], ["x3"])], [W.tensor("s", np.asarray([-1, 5, 16], np.int64)), W.tensor("w", np.ones((16, 3), np.float32))]
    out = W.rotary_op_nodes(nodes, inits, "r_", "x3", *W.rotary_tables(5, 8), num_heads=2)
    nodes.append(W.node("MatMul", [out, "w"], ["y"]))
    p = plan_of(api, tmp_path, W.model("m", nodes, inits, [W.value_info("X", ["N", 80])], [W.value_info("y", ["N", 5, 3])], opset=23))
    assert kinds(p) == ["Rotary", "Dense"] and p["steps"][0]["form"] == "vec4"


# (the spelling sits on a head-major value: there is none in front of the operator's 3-D operands)
FRONTS = [(f, s) for f in ("operator_4d", "operator_3d", "pattern") for s in ("op", "slice", "split") if f != "operator_3d" or s == "op"]


@pytest.mark.parametrize("front,spelling", FRONTS)
def test_one_rotary_step_per_rotated_operand_in_front_of_one_attention(api, tmp_path, front, spelling):
    rot = {"form": spelling}
    if front == "pattern":
        blob = W.attention_only(T, HQ * DH, HQ, form="three", k_transpose="two_step", rotary=rot, opset=23)
        hkv = HQ
    elif front == "operator_3d":
        blob, hkv = W.attention_op_model(T, T, HQ, HKV, DH, form="3d", causal=True, rotary=rot), HKV
    else:
        blob, hkv = W.attention_op_model(T, T, HQ, HKV, DH, form="4d", causal=True, rotary=rot), HKV
    p = plan_of(api, tmp_path, blob)
    assert kinds(p) == ["SliceCols"] * 3 + ["Rotary", "Rotary", "Attention"], kinds(p)
    q, k = rotary_steps(p)
    att = p["steps"][-1]
    for s, h in ((q, HQ), (k, hkv)):
        assert (s["T"], s["heads"], s["dh"], s["rd"], s["interleaved"], s["positions"], s["form"]) == (T, h, DH, DH, False, "arange", "vec4"), s
    assert (att["in"], att["in1"]) == (q["out"], k["out"]) and att["heads"] == HQ and att["dh"] == DH
    assert p["flops_per_row"] == 4 * T * T * HQ * DH + 3 * T * (HQ + hkv) * DH
    want = {"op": "RotaryEmbedding:a_q_rope", "slice": "Slice:a_q_slice1+...+Add:a_q_add", "split": "Split:a_q_split+...+Add:a_q_add"}[spelling]
    assert q["origin"] == want, q["origin"]


@pytest.mark.parametrize("front", ["operator", "pattern"])
def test_operator_and_spelling_give_equal_plans(api, tmp_path, front):
    plans = []
    for rot in ({"form": "op"}, {"form": "slice"}, {"form": "split"}, {"form": "slice", "slice_end": "max", "swap": True, "table_rank": 4}, {"form": "split", "table_rank": 3}):
        blob = (W.attention_op_model(T, T, HQ, HKV, DH, causal=True, rotary=rot) if front == "operator" else
                W.attention_only(T, HQ * DH, HQ, k_transpose="two_step", rotary=rot, opset=23))
        plans.append(plan_of(api, tmp_path, blob))
    first = [without(s, "origin") for s in plans[0]["steps"]]
    for p in plans[1:]:
        assert [without(s, "origin") for s in p["steps"]] == first
    assert len(rotary_steps(plans[0])) == 2 and plans[0]["flops_per_row"] == plans[1]["flops_per_row"]


@pytest.mark.parametrize("spelling", ["op", "slice"])
def test_the_packed_projection_is_still_read_in_place(api, tmp_path, spelling):
    E = HQ * DH
    for blob in (W.attention_op_model(T, T, HQ, HQ, DH, packed=True, rotary={"form": spelling}),
                 W.attention_only(T, E, HQ, k_transpose="two_step", rotary={"form": spelling}, opset=23)):
        p = plan_of(api, tmp_path, blob)
        assert kinds(p) == ["Rotary", "Rotary", "Attention"], kinds(p)  # no SliceCols for Q or K: the cuts are views
        q, k = rotary_steps(p)
        assert (q["in"], q["ld"], q["off"]) == (0, 3 * E, 0) and (k["in"], k["ld"], k["off"]) == (0, 3 * E, E)
        att = p["steps"][-1]
        assert (att["in"], att["in1"], att["in2"]) == (q["out"], k["out"], 0)
    # K at column 18 of a row of 54: no 16-byte alignment, the scalar form
    p = plan_of(api, tmp_path, W.attention_op_model(5, 5, 3, 3, 6, packed=True, rotary={"form": spelling}))
    assert [(s["off"], s["form"]) for s in rotary_steps(p)] == [(0, "scalar"), (18, "scalar")]


def test_merged_projections_are_rotated_where_they_lie(api, tmp_path):
    """three private window Dense projections of one value become one packed Dense; Q and K are rotated out of it"""
    E = 16
    rng = np.random.default_rng(0)
    nodes, inits = [W.node("Reshape", ["X", "s"], ["x3"])], [W.tensor("s", np.asarray([-1, T, E], np.int64))]
    for c in "qkv":
        inits.append(W.tensor("w" + c, rng.uniform(-1, 1, (E, E)).astype(np.float32)))
        nodes.append(W.node("MatMul", ["x3", "w" + c], [c]))
    out = W.attention_op_nodes(nodes, inits, "a_", "q", "k", "v", T, T, 2, 2, 8, rotary=True)
    p = plan_of(api, tmp_path, W.model("m", nodes, inits, [W.value_info("X", ["N", T * E])], [W.value_info(out, ["N", T, E])], opset=23))
    assert kinds(p) == ["Dense", "Rotary", "Rotary", "Attention"], kinds(p)
    assert [(s["ld"], s["off"]) for s in rotary_steps(p)] == [(3 * E, 0), (3 * E, E)]


def test_decoder_block_plan_with_rotary(api, tmp_path):
    spec = W.decoder_block_spec(rotary=True)
    for form in ("4d", "3d"):
        for rot in (None, {"form": "split"}) if form == "4d" else (None,):
            p = plan_of(api, tmp_path, W.decoder_block_from_spec(spec, form=form, rotary=rot))
            per_layer = ["RmsNorm", "Dense", "Dense", "Dense", "Rotary", "Rotary", "Attention", "Dense", "BinaryAct", "RmsNorm", "Dense", "Dense", "BinaryAct", "Dense",
                         "BinaryAct"]
            assert kinds(p) == per_layer * 2 + ["RmsNorm", "SliceCols", "Dense"], kinds(p)
            rots = rotary_steps(p)
            assert [s["heads"] for s in rots] == [spec["hq"], spec["hkv"]] * 2 and len({s["tables_hash"] for s in rots}) == 1
            att = [s for s in p["steps"] if s["kind"] == "Attention"]
            assert all(s["causal"] is True and s["kv_heads"] == spec["hkv"] for s in att)


def test_one_rotated_value_read_as_two_operands_is_rotated_once(api, tmp_path):
    """Attention(rope(q), rope(k), rope(k)): K and V are ONE rotated value, one Rotary step"""
    nodes, inits = [], []
    for nm, h in (("q", HQ), ("k", HKV)):
        inits += [W.tensor(nm + "_shape", np.asarray([-1, T, h * DH], np.int64)), W.tensor(nm + "_split", np.asarray([0, T, h, DH], np.int64))]
        nodes += [W.node("Reshape", [nm.upper(), nm + "_shape"], [nm]), W.node("Reshape", [nm, nm + "_split"], [nm + "4"]),
                  W.node("Transpose", [nm + "4"], [nm + "h"], [W.attr_ints("perm", [0, 2, 1, 3])])]
    qr = W.rotary_op_nodes(nodes, inits, "q_", "qh", *W.rotary_tables(T, DH))
    kr = W.rotary_op_nodes(nodes, inits, "k_", "kh", *W.rotary_tables(T, DH))
    inits.append(W.tensor("merge", np.asarray([0, T, HQ * DH], np.int64)))
    nodes += [W.node("Attention", [qr, kr, kr], ["y4"], name="attn"), W.node("Transpose", ["y4"], ["yt"], [W.attr_ints("perm", [0, 2, 1, 3])]),
              W.node("Reshape", ["yt", "merge"], ["y"])]
    ins = [W.value_info("Q", ["N", T * HQ * DH]), W.value_info("K", ["N", T * HKV * DH])]
    p = plan_of(api, tmp_path, W.model("m", nodes, inits, ins, [W.value_info("y", ["N", T, HQ * DH])], opset=23))
    assert kinds(p) == ["SliceCols", "SliceCols", "Rotary", "Rotary", "Attention"], kinds(p)
    att, (q, k) = p["steps"][-1], rotary_steps(p)
    assert (att["in"], att["in1"], att["in2"]) == (q["out"], k["out"], k["out"])


def test_constant_positions_are_gathered_at_load(api, tmp_path):
    pos = [6, 0, 9, 3, 3]
    p = plan_of(api, tmp_path, W.rotary_model(5, 2, 8, rotary={"positions": pos, "cache_rows": 12}))
    cos, sin = W.rotary_tables(12, 8)
    nodes, inits = [W.node("Reshape", ["X", "s"], ["x3"])], [W.tensor("s", np.asarray([-1, 5, 16], np.int64))]
    out = W.rotary_op_nodes(nodes, inits, "r_", "x3", cos[pos], sin[pos], num_heads=2)
    by_hand = plan_of(api, tmp_path, W.model("m", nodes, inits, [W.value_info("X", ["N", 80])], [W.value_info(out, ["N", 5, 16])], opset=23))
    a, b = p["steps"][0], by_hand["steps"][0]
    assert (a["positions"], b["positions"]) == ("constant", "arange")
    assert without(a, "positions") == without(b, "positions")
    assert a["tables_hash"] != plan_of(api, tmp_path, W.rotary_model(5, 2, 8))["steps"][0]["tables_hash"]


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------

def op_model(T_=5, h=2, dh=8, cos=None, sin=None, x_rank=3, attrs=(), num_heads=None, positions=None, inputs=(), pos_name=None, opset=23, domain="",
             cos_name=None, reader="output"):
    """RotaryEmbedding 'rope' by hand.  x_rank 3: X [N, T, h dh]; 4: the head split of it, the result read by `reader`: "relu" (no attention
    operand), or, x_rank "input4": a head-major graph input"""
    E = h * dh
    c, s = W.rotary_tables(T_, dh)
    cos = c[None] if cos is None else cos
    sin = s[None] if sin is None else sin
    nodes, inits = [W.node("Reshape", ["X", "s3"], ["x3"])], [W.tensor("s3", np.asarray([-1, T_, E], np.int64)), W.tensor("sin", np.asarray(sin, np.float32))]
    if cos_name is None:
        inits.append(W.tensor("cos", np.asarray(cos, np.float32)))
    ins = [W.value_info("X", ["N", T_ * E])] + list(inputs)
    x = "x3"
    if x_rank == 4:
        inits.append(W.tensor("s4", np.asarray([0, T_, h, dh], np.int64)))
        nodes += [W.node("Reshape", ["x3", "s4"], ["x4"]), W.node("Transpose", ["x4"], ["xh"], [W.attr_ints("perm", [0, 2, 1, 3])])]
        x = "xh"
    a = list(attrs) + ([W.attr_i("num_heads", h if num_heads is None else num_heads)] if (x_rank == 3 and num_heads != 0) else [])
    rin = [x, cos_name or "cos", "sin"]
    if positions is not None:
        inits.append(W.tensor("pos", np.asarray(positions, np.int64)))
        rin.append("pos")
    if pos_name:
        rin.append(pos_name)
    nodes.append(W.node("RotaryEmbedding", rin, ["r"], a, name="rope", domain=domain))
    out, oshape = "r", ["N", T_, E]
    if x_rank == 4:
        nodes.append(W.node("Relu", ["r"], ["y"]))
        out, oshape = "y", ["N", h, T_, dh]
    return W.model("m", nodes, inits, ins, [W.value_info(out, oshape)], opset=opset)


NAMED = "node 'rope' (RotaryEmbedding): unsupported operator form: "


def test_refusals_name_the_node(api, tmp_path):
    c, s = W.rotary_tables(5, 8)
    c12, s12 = W.rotary_tables(12, 8)
    cases = {
        "a position outside the caches": (op_model(cos=c12, sin=s12, positions=[[0, 1, 12, 3, 4]]), "position 12"),
        "a negative position": (op_model(cos=c12, sin=s12, positions=[[0, 1, -1, 3, 4]]), "position -1"),
        "per-row positions": (op_model(cos=c12, sin=s12, pos_name="P", inputs=[W.value_info("P", ["N", 5], W.INT64)]), "per-row positions are not supported yet"),
        "non-constant caches": (op_model(cos_name="C", inputs=[W.value_info("C", ["N", 20])]), "is not a constant"),
        "a leading extent other than 1": (op_model(cos=np.stack([c, c]), sin=np.stack([s, s])), "leading extent of 2"),
        "a cache width that is not rd/2": (op_model(cos=c[None, :, :3], sin=s[None, :, :3]), "rd/2 columns"),
        "odd rd": (op_model(attrs=[W.attr_i("rotary_embedding_dim", 3)]), "rotary_embedding_dim = 3 must be even"),
        "rd > dh": (op_model(attrs=[W.attr_i("rotary_embedding_dim", 10)]), "rotary_embedding_dim = 10 must be even and at most the head size 8"),
        "3-D X without num_heads": (op_model(num_heads=0), "a 3-D X needs num_heads"),
        "E % num_heads": (op_model(num_heads=3), "E = 16 is not divisible by num_heads = 3"),
        "4-D result read by something else": (op_model(x_rank=4), "its 4-D result is read by something other than an attention operand"),
        "interleaved = 2": (op_model(attrs=[W.attr_i("interleaved", 2)]), "interleaved = 2"),
        "opset 22": (op_model(opset=22), "from opset 23 on"),
        "caches of other T": (op_model(cos=c[None, :4], sin=s[None, :4]), "the caches hold 4 steps, the window T = 5"),
    }
    for what, (blob, text) in cases.items():
        err = load_error(api, tmp_path, blob)
        assert NAMED in err and text in err, (what, err)


def test_head_major_and_capped_forms_are_refused_by_name(api, tmp_path):
    # a 4-D X that is not a head split: a head-major graph input in front of the Attention operator
    nodes, inits = [W.node("Reshape", ["X", "s4"], ["q4"]), W.node("Reshape", ["X", "s4"], ["k4"])], [W.tensor("s4", np.asarray([-1, 2, T, DH], np.int64))]
    c, s = W.rotary_tables(T, DH)
    q = W.rotary_op_nodes(nodes, inits, "q_", "q4", c, s)
    nodes.append(W.node("Attention", [q, "k4", "k4"], ["y"], name="attn"))
    err = load_error(api, tmp_path, W.model("m", nodes, inits, [W.value_info("X", ["N", 2 * T * DH])], [W.value_info("y", ["N", 2, T, DH])], opset=23))
    assert "node 'q_rope' (RotaryEmbedding): unsupported operator form: its 4-D X is not the head split" in err, err
    # the caps are the attention kernel's
    err = load_error(api, tmp_path, W.rotary_model(1025, 1, 2))
    assert "node 'r_rope' (RotaryEmbedding)" in err and "T = 1025 is beyond the Rotary kernel's cap of 1024" in err, err
    err = load_error(api, tmp_path, W.rotary_model(2, 1, 130))
    assert "node 'r_rope' (RotaryEmbedding)" in err and "dh = 130 is beyond the Rotary kernel's cap of 128" in err, err
    err = load_error(api, tmp_path, W.rotary_model(1, 1025, 2))
    assert "node 'r_rope' (RotaryEmbedding)" in err and "h = 1025 is beyond the Rotary kernel's cap of 1024" in err, err
    # the contrib-domain operator
    err = load_error(api, tmp_path, W.rotary_model(5, 2, 8, domain="com.microsoft"))
    assert "node 'r_rope' (RotaryEmbedding)" in err and "contrib RotaryEmbedding of domain 'com.microsoft' is not supported" in err, err


def test_num_heads_that_disagrees_with_the_head_split_is_refused(api, tmp_path):
    nodes, inits = [], []
    for nm in "qkv":
        inits.append(W.tensor(nm + "_shape", np.asarray([-1, T, HQ * DH], np.int64)))
        nodes.append(W.node("Reshape", [nm.upper(), nm + "_shape"], [nm]))

    def blob(extra):
        n, i = list(nodes), list(inits)
        i += [W.tensor("s4", np.asarray([0, T, HQ, DH], np.int64)), W.tensor("merge", np.asarray([0, T, HQ * DH], np.int64))]
        heads = {}
        for nm in "qkv":
            n += [W.node("Reshape", [nm, "s4"], [nm + "4"]), W.node("Transpose", [nm + "4"], [nm + "h"], [W.attr_ints("perm", [0, 2, 1, 3])])]
            heads[nm] = nm + "h"
        heads["q"] = W.rotary_op_nodes(n, i, "r_", "qh", *W.rotary_tables(T, DH), extra_attrs=extra)
        n += [W.node("Attention", [heads["q"], heads["k"], heads["v"]], ["y4"], name="attn"),
              W.node("Transpose", ["y4"], ["yt"], [W.attr_ints("perm", [0, 2, 1, 3])]), W.node("Reshape", ["yt", "merge"], ["y"])]
        ins = [W.value_info(nm, ["N", T * HQ * DH]) for nm in "QKV"]
        return W.model("m", n, i, ins, [W.value_info("y", ["N", T, HQ * DH])], opset=23)

    p = plan_of(api, tmp_path, blob([W.attr_i("num_heads", HQ)]))  # the attribute beside a 4-D X, in agreement: served
    assert kinds(p) == ["SliceCols"] * 3 + ["Rotary", "Attention"], kinds(p)
    err = load_error(api, tmp_path, blob([W.attr_i("num_heads", HQ // 2)]))
    assert "node 'r_rope' (RotaryEmbedding): unsupported operator form: num_heads = 2 disagrees with the 4 heads of the head split" in err, err


def test_rotate_half_tables_of_another_shape_are_refused_by_name(api, tmp_path):
    """the spelling is matched by structure before shapes are known; tables that are not [T, dh] are then refused at its Add"""
    E = HQ * DH
    nodes, inits = [], [W.tensor("x_shape", np.asarray([-1, T, E], np.int64))]
    for nm in "qkv":
        nodes.append(W.node("Reshape", [nm.upper(), "x_shape"], [nm]))
    ins = [W.value_info(nm, ["N", T * E]) for nm in "QKV"]
    for rows in (T + 1, 1):  # another T; a [1, dh] table that would broadcast over the steps
        n, i = list(nodes), list(inits)
        cos, sin = W.rotary_tables(rows, DH)
        # attention_nodes with the tables swapped in: build the spelling on Q by hand in front of the pattern
        i += [W.tensor("a_split", np.asarray([0, T, HQ, DH], np.int64)), W.tensor("a_merge", np.asarray([0, T, E], np.int64)),
              W.tensor("a_sc", np.asarray(0.25, np.float32))]
        n += [W.node("Reshape", ["q", "a_split"], ["q4"]), W.node("Transpose", ["q4"], ["qh"], [W.attr_ints("perm", [0, 2, 1, 3])]),
              W.node("Reshape", ["k", "a_split"], ["k4"]), W.node("Transpose", ["k4"], ["kh"], [W.attr_ints("perm", [0, 2, 3, 1])]),
              W.node("Reshape", ["v", "a_split"], ["v4"]), W.node("Transpose", ["v4"], ["vh"], [W.attr_ints("perm", [0, 2, 1, 3])])]
        qr = W.rotate_half_nodes(n, i, "r_", "qh", np.concatenate([cos, cos], axis=1), np.concatenate([sin, sin], axis=1))
        n += [W.node("MatMul", [qr, "kh"], ["s0"], name="a_qk"), W.node("Mul", ["s0", "a_sc"], ["s1"]), W.node("Softmax", ["s1"], ["pr"], [W.attr_i("axis", -1)]),
              W.node("MatMul", ["pr", "vh"], ["o4"]), W.node("Transpose", ["o4"], ["ot"], [W.attr_ints("perm", [0, 2, 1, 3])]),
              W.node("Reshape", ["ot", "a_merge"], ["y"], name="a_merge_heads")]
        err = load_error(api, tmp_path, W.model("m", n, i, ins, [W.value_info("y", ["N", T, E])], opset=20))
        assert "node 'r_add' (Add): unsupported operator form: the rotate_half tables must be [T, dh] = [8,8]" in err, err


def test_float16_rotary_is_refused(api, tmp_path):
    c, s = W.rotary_tables(5, 8)
    nodes, inits = [W.node("Reshape", ["X", "s3"], ["x3"])], [W.tensor("s3", np.asarray([-1, 5, 16], np.int64)),
                                                             W.tensor("r_cos", c[None].astype(np.float16)), W.tensor("r_sin", s[None].astype(np.float16))]
    nodes.append(W.node("RotaryEmbedding", ["x3", "r_cos", "r_sin"], ["r"], [W.attr_i("num_heads", 2)], name="rope"))
    blob = W.model("m", nodes, inits, [W.value_info("X", ["N", 80], W.FLOAT16)], [W.value_info("r", ["N", 5, 16], W.FLOAT16)], opset=23)
    err = load_error(api, tmp_path, blob)
    assert NAMED in err and "float16" in err, err


# ---- a sub-graph that is not exactly the spelling is refused as before ----------------------------------------------------------------------

GENERIC = ("node 'a_qk' (MatMul): unsupported operator form: MatMul of two activations outside a recognised self-attention pattern (Reshape [N,T,h,dh] -> "
           "Transpose(0,2,1,3), Q K^T, scale, constant mask, Softmax(-1), P V, Transpose(0,2,1,3) -> Reshape [N,T,E]); the right operand must otherwise be a "
           "constant weight matrix")


def second_reader_model():
    """the exact spelling on Q, whose x has one more reader (a Relu that reaches the output)"""
    E = HQ * DH
    nodes, inits = [], [W.tensor("x_shape", np.asarray([-1, T, E], np.int64))]
    for nm in "qkv":
        nodes.append(W.node("Reshape", [nm.upper(), "x_shape"], [nm]))
    out = W.attention_nodes(nodes, inits, "a_", "q", "k", "v", "q", T, E, HQ, k_transpose="two_step", rotary={"form": "slice", "on": "q"})
    nodes += [W.node("Relu", ["a_qh"], ["extra4"]), W.node("Transpose", ["extra4"], ["extra_t"], [W.attr_ints("perm", [0, 2, 1, 3])]),
              W.node("Reshape", ["extra_t", "a_merge"], ["extra"]), W.node("Add", [out, "extra"], ["y"])]
    return W.model("m", nodes, inits, [W.value_info(nm, ["N", T * E]) for nm in "QKV"], [W.value_info("y", ["N", T, E])], opset=20)


def test_a_broken_rotate_half_is_refused_as_before(api, tmp_path):
    E = HQ * DH
    broken = {
        "wrong slice bounds": W.attention_only(T, E, HQ, form="three", k_transpose="two_step", rotary={"form": "slice", "break_": "bounds"}),
        "Concat order x1, -x2": W.attention_only(T, E, HQ, form="three", k_transpose="two_step", rotary={"form": "slice", "break_": "order"}),
        "Concat order x1, -x2 (Split)": W.attention_only(T, E, HQ, form="three", k_transpose="two_step", rotary={"form": "split", "break_": "order"}),
        "x with a second reader": second_reader_model(),
    }
    for what, blob in broken.items():
        err = load_error(api, tmp_path, blob)
        assert GENERIC in err, (what, err)
    # the same spelling, unbroken and on Q alone, loads
    p = plan_of(api, tmp_path, W.attention_only(T, E, HQ, form="three", k_transpose="two_step", rotary={"form": "slice", "on": "q"}))
    assert kinds(p) == ["SliceCols"] * 3 + ["Rotary", "Attention"], kinds(p)


# ---- with default arguments the writers emit what they emitted before ----------------------------------------------------------------------

# sha256 of the writers' output on the commit before the rotary= keyword
DIGESTS = {
    "attention_op_model 4d": "9639356c50b13c9152655f012f7bd3b66a2f7683d626dc402dcdb37bc7ea49d0",
    "attention_op_model 3d causal": "727504b02aa1953f09829f8e11948bdfbc5aa23d2b6a46928e2dcc63cba5ab01",
    "attention_op_model packed": "c82998aede2a2b39437f6e592f7b362a98c7585a764df7d544c26fd6a0b61332",
    "attention_only packed": "ef716f4b875f9aa9c0551fc2f7d1756e4a378540234f68324044b10d18dfa38b",
    "attention_only three two_step": "c2263d1c230baf01aa4dccddc6e2fb07b44f384d1fd7e055b5e8ab211c68fea4",
    "decoder_block_from_spec 4d": "4df3036f018963fb95ff4c2fcac61d093273e82cc90aa0874579281ce4928b04",
    "decoder_block_from_spec 3d": "aae7434aec0bff38a340603d78c6ea9f53a4c5dae17e04ea434076b714775dac",
}


def test_default_arguments_emit_byte_identical_models():
    spec = W.decoder_block_spec()
    assert "rotary" not in spec
    got = {
        "attention_op_model 4d": W.attention_op_model(5, 5, 4, 2, 8),
        "attention_op_model 3d causal": W.attention_op_model(5, 7, 4, 2, 8, form="3d", causal=True),
        "attention_op_model packed": W.attention_op_model(5, 5, 2, 2, 8, packed=True),
        "attention_only packed": W.attention_only(6, 16, 2),
        "attention_only three two_step": W.attention_only(6, 16, 2, form="three", k_transpose="two_step"),
        "decoder_block_from_spec 4d": W.decoder_block_from_spec(spec),
        "decoder_block_from_spec 3d": W.decoder_block_from_spec(spec, form="3d"),
    }
    assert {k: hashlib.sha256(v).hexdigest() for k, v in got.items()} == DIGESTS
    assert W.attention_op_model(5, 5, 4, 2, 8, rotary=None) == got["attention_op_model 4d"]
    assert W.attention_op_model(5, 5, 4, 2, 8, rotary=True) != got["attention_op_model 4d"]
