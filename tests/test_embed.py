"""Embedding lookups without a GPU: what the loader recognises as the Embed step (Gather of a constant f32 table by runtime indices, the
column picks, Casts and offset Adds in front of it, the Reshape / Flatten and feature-axis Concat behind it), the plans it makes of the four
spellings of infera_amd.onnx_writer.embedding_from_spec, and what it refuses (INTEGRATION.md 2.6 "Embedding lookups").
"""
import os

import numpy as np
import pytest

from infera_amd import onnx_writer as W


@pytest.fixture(scope="module")
def api(built):
    from infera_amd import capi

    return capi


def plan_of(api, tmp_path, blob, name="emb", info=False):
    path = W.write(os.path.join(str(tmp_path), name + ".onnx"), blob)
    api.load_model(name, path)
    try:
        return (api.get_plan(name), api.get_model_info(name)) if info else api.get_plan(name)
    finally:
        api.unload_model(name)


def load_error(api, tmp_path, blob, name="bad"):
    path = W.write(os.path.join(str(tmp_path), name + ".onnx"), blob)
    with pytest.raises(Exception) as e:
        api.load_model(name, path)
        api.unload_model(name)
    return str(e.value)


def kinds(plan):
    return [s["kind"] for s in plan["plan"]["steps"]]


def lookup(V, d, src, out, table=0, offset=0):
    return {"table": table, "src": src, "V": V, "d": d, "offset": offset, "out": out}


def i64(name, v):
    return W.tensor(name, np.asarray(v, dtype=np.int64))


ENCODER_LAYER = ["Dense", "Attention", "Dense", "BinaryAct", "LayerNorm", "Dense", "Dense", "BinaryAct", "LayerNorm"]  # (post-norm, merged Q K V)


def encoder(T, E, pos):
    enc = W.transformer_spec(T=T, F=E, E=E, h=2, ff=16, layers=2)
    enc["Win"] = enc["bin"] = None  # (the window is the encoder's input: no projection)
    if not pos:
        enc["pos"] = None
    return enc


# ---- the four spellings ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spelling,front", [("a", {}), ("a", {"pick": "slice"}), ("a", {"int_type": W.INT32}), ("d", {}), ("d", {"pick": "slice"})])
def test_per_column_tables_into_an_mlp(api, tmp_path, spelling, front):
    """(a) / (d): tables of d = 3, 4, 2, then 2 numeric columns: ONE Embed step in front of the MLP, no Prep, SliceCols or CopyCols beside it"""
    spec = W.embedding_spec(cards=(7, 11, 5), dims=(3, 4, 2), numeric=2, hidden=(16, 8))
    plan, info = plan_of(api, tmp_path, W.embedding_from_spec(spec, spelling, **front), info=True)
    assert kinds(plan) == ["Embed", "Dense", "Dense", "Dense"]
    s = plan["plan"]["steps"][0]
    assert s["pieces"] == [lookup(7, 3, 0, 0, 0), lookup(11, 4, 1, 3, 1), lookup(5, 2, 2, 7, 2), {"copy": 2, "src": 3, "out": 9}]
    assert (s["in"], s["W"], s["out_cols"], s["window"]) == (0, 5, 11, None)
    assert s["bytes_per_row"] == 4 * (5 + 9 + 11)  # the source columns, the gathered floats, the written row
    for nm in ("Gather:emb0", "Gather:emb1", "Gather:emb2", "Concat:join") + (("Cast:cast1", "Slice:numeric") if spelling == "d" else ()):
        assert nm in s["origin"].split("+"), s["origin"]
    assert (plan["plan"]["steps"][1]["in"], plan["plan"]["steps"][1]["K"]) == (s["out"], 11)
    assert plan["plan"]["flops_per_row"] == 2 * (11 * 16 + 16 * 8 + 8 * 1)  # (the lookup adds nothing)
    assert info["input_shape"] == [-1, 5] and info["output_shape"] == [-1, 1]
    assert plan["plan"]["input_shape"] == [-1, 5] and plan["plan"]["output_shape"] == [-1, 1]


@pytest.mark.parametrize("offsets_rank", [1, 2])
def test_shared_table_with_offsets(api, tmp_path, offsets_rank):
    """(b): one table, the per-column offsets folded into the pieces; flattened into an MLP, and as a window into an encoder"""
    spec = W.embedding_spec(cards=(7, 11, 5, 3), dims=8, numeric=0, hidden=(16,))
    V = 26
    pieces = [lookup(V, 8, j, 8 * j, 0, off) for j, off in enumerate((0, 7, 18, 23))]
    for flatten in ("reshape", "flatten"):
        plan = plan_of(api, tmp_path, W.embedding_from_spec(spec, "b", flatten=flatten, offsets_rank=offsets_rank))
        assert kinds(plan) == ["Embed", "Dense", "Dense"]
        s = plan["plan"]["steps"][0]
        assert (s["pieces"], s["out_cols"], s["window"], s["tables"]) == (pieces, 32, None, 1)
        assert s["origin"] == ("Add:offset+Gather:emb+" + ("Reshape" if flatten == "reshape" else "Flatten") + ":flatten")
    plan, info = plan_of(api, tmp_path, W.embedding_from_spec(spec, "b", tail="encoder", encoder=encoder(4, 8, False), flatten="window", offsets_rank=offsets_rank), info=True)
    assert kinds(plan) == ["Embed"] + 2 * ENCODER_LAYER + ["MeanTime", "Dense"]
    s = plan["plan"]["steps"][0]
    assert (s["pieces"], s["out_cols"], s["window"]) == (pieces, 32, [4, 8])
    assert plan["plan"]["steps"][1]["T"] == 4 and plan["plan"]["steps"][2]["T"] == 4  # the window Dense and the attention over its 4 steps
    assert info["input_shape"] == [-1, 4] and info["output_shape"] == [-1, 1]


def test_token_ids_into_position_add_encoder_and_mean(api, tmp_path):
    """(c): Gather(table, ids [N, T]) is a flat window [rows, T, d]: positional Add -> encoder layers -> MeanTime -> head"""
    spec = W.embedding_spec(cards=(50,) * 6, dims=8, numeric=0, hidden=())
    plan, info = plan_of(api, tmp_path, W.embedding_from_spec(spec, "c", tail="encoder", encoder=encoder(6, 8, True)), info=True)
    assert kinds(plan) == ["Embed", "BinaryConst"] + 2 * ENCODER_LAYER + ["MeanTime", "Dense"]
    s = plan["plan"]["steps"][0]
    assert s["pieces"] == [lookup(50, 8, t, 8 * t) for t in range(6)]
    assert (s["out_cols"], s["window"], s["origin"]) == (48, [6, 8], "Gather:emb")
    assert info["input_shape"] == [-1, 6] and info["output_shape"] == [-1, 1]
    # the window alone is the output [N, T, d]; one time step of it is cut out as behind a recurrent step
    plan = plan_of(api, tmp_path, W.embedding_from_spec(spec, "c", tail="none"))
    assert kinds(plan) == ["Embed"] and plan["plan"]["output_shape"] == [-1, 6, 8]
    nodes, inits, cur, _, inputs = W.embedding_nodes(spec, "c")
    nodes.append(W.node("Gather", [cur, "last"], ["Y"], [W.attr_i("axis", 1)], name="last_step"))
    plan = plan_of(api, tmp_path, W.model("last", nodes, inits + [i64("last", -1)], inputs, [W.value_info("Y", ["N", 8])]))
    assert kinds(plan) == ["Embed", "SliceCols"] and plan["plan"]["output_shape"] == [-1, 8]


def test_rank1_table_and_single_lookup(api, tmp_path):
    spec = W.embedding_spec(cards=(9,), dims=(1,), numeric=0, hidden=(), table_rank1=True)
    nodes, inits, cur, _, inputs = W.embedding_nodes(spec, "a", concat=False)
    assert cur == "e0"
    plan = plan_of(api, tmp_path, W.model("r1", nodes, inits, inputs, [W.value_info("e0", ["N", 1])]))
    assert kinds(plan) == ["Embed"]
    s = plan["plan"]["steps"][0]
    assert s["pieces"] == [lookup(9, 1, 0, 0)] and s["out_cols"] == 1 and plan["plan"]["output_shape"] == [-1, 1]
    # ids [N, k] into a [V] table: [N, k], a feature row
    nodes = [W.node("Gather", ["t", "x_cat"], ["Y"], name="emb")]
    plan = plan_of(api, tmp_path, W.model("r1k", nodes, [W.tensor("t", np.arange(5, dtype=np.float32))], [W.value_info("x_cat", ["N", 3], W.INT64)], [W.value_info("Y", ["N", 3])]))
    assert kinds(plan) == ["Embed"] and plan["plan"]["steps"][0]["window"] is None and plan["plan"]["output_shape"] == [-1, 3]


# ---- where the old machinery keeps its part ------------------------------------------------------------------------------------------------
def test_scaler_on_the_numeric_columns_keeps_its_steps(api, tmp_path):
    """A Scaler between x_num and the Concat is more than a copy: it stays the AffineChannel behind the input's SliceCols, ONE Embed step
    serves the three lookups and leaves a gap of two columns in its row, and one CopyCols (allowed here) puts the scaled columns there."""
    spec = W.embedding_spec(cards=(7, 11, 5), dims=(3, 4, 2), numeric=2, hidden=())
    nodes, inits, _, _, inputs = W.embedding_nodes(spec, "a")
    nodes = [n for n in nodes if b"join" not in n]
    nodes.append(W.node("Scaler", ["x_num"], ["x_s"], [W.attr_floats("offset", [0.5, 1.0]), W.attr_floats("scale", [2.0, 3.0])], name="scale", domain=W.ML_DOMAIN))
    for order in (["e0", "e1", "e2", "x_s"], ["e0", "x_s", "e1", "e2"]):
        blob = W.model("mixed", nodes + [W.node("Concat", order, ["Y"], [W.attr_i("axis", 1)], name="join")], inits, inputs, [W.value_info("Y", ["N", 11])], ml_opset=3)
        plan = plan_of(api, tmp_path, blob)
        assert kinds(plan) == ["SliceCols", "AffineChannel", "Embed", "CopyCols"]
        _, scaled, emb, copy = plan["plan"]["steps"]
        if order[-1] == "x_s":
            assert emb["pieces"] == [lookup(7, 3, 0, 0, 0), lookup(11, 4, 1, 3, 1), lookup(5, 2, 2, 7, 2), {"gap": 2, "out": 9}]
        else:
            assert emb["pieces"] == [lookup(7, 3, 0, 0, 0), {"gap": 2, "out": 3}, lookup(11, 4, 1, 5, 1), lookup(5, 2, 2, 9, 2)]
        assert (emb["in"], emb["W"], emb["out_cols"]) == (0, 5, 11)
        assert (copy["in"], copy["out"], copy["origin"]) == (scaled["out"], emb["out"], "Concat:join[%d]" % order.index("x_s"))
        assert plan["plan"]["output_shape"] == [-1, 11]


def _shared_index_model(second_reader):
    t1, t2 = np.arange(12, dtype=np.float32).reshape(4, 3), np.arange(8, dtype=np.float32).reshape(4, 2)
    nodes = [W.node("Gather", ["x_cat", "c1"], ["col"], [W.attr_i("axis", 1)], name="pick"), W.node("Gather", ["t1", "col"], ["a"], name="emb_a"),
             W.node("Gather", ["t2", "col"], ["b"], name="emb_b")]
    parts = ["a", "b"]
    if second_reader:
        nodes.append(W.node("Relu", ["a"], ["ar"], name="relu"))
        parts.append("ar")
    nodes.append(W.node("Concat", parts, ["Y"], [W.attr_i("axis", 1)], name="join"))
    return W.model("shared", nodes, [W.tensor("t1", t1), W.tensor("t2", t2), i64("c1", 1)], [W.value_info("x_cat", ["N", 2], W.INT64)],
                   [W.value_info("Y", ["N", 8 if second_reader else 5])])


def test_two_lookups_of_one_index_and_a_second_reader(api, tmp_path):
    """Two tables looked up by ONE index value: one step, two pieces that read the same source column.  A lookup that a Relu reads too: the
    Concat's step still holds both lookups (looking a row up twice costs no pass) and a gap that one CopyCols fills with the Relu's result;
    the Relu reads a step of that one lookup alone."""
    plan = plan_of(api, tmp_path, _shared_index_model(False))
    assert kinds(plan) == ["Embed"]
    s = plan["plan"]["steps"][0]
    assert s["pieces"] == [lookup(4, 3, 1, 0, 0), lookup(4, 2, 1, 3, 1)] and s["origin"] == "Gather:pick+Gather:emb_a+Gather:emb_b+Concat:join"
    plan = plan_of(api, tmp_path, _shared_index_model(True))
    assert kinds(plan) == ["Embed", "Unary", "Embed", "CopyCols"]
    a, relu, cat, copy = plan["plan"]["steps"]
    assert a["pieces"] == [lookup(4, 3, 1, 0)] and a["origin"] == "Gather:pick+Gather:emb_a" and relu["in"] == a["out"]
    assert cat["pieces"] == [lookup(4, 3, 1, 0, 0), lookup(4, 2, 1, 3, 1), {"gap": 3, "out": 5}] and cat["in"] == 0
    assert (copy["in"], copy["out"], copy["origin"]) == (relu["out"], cat["out"], "Concat:join[2]")
    assert plan["plan"]["output_shape"] == [-1, 8]


def test_rank1_tables_through_unsqueeze_are_one_step(api, tmp_path):
    """spelling (a) with [V] tables: every lookup is [N], an Unsqueeze makes it [N, 1] for the Concat; all of it is one step"""
    spec = W.embedding_spec(cards=(9, 4, 6), dims=(1, 1, 1), numeric=1, hidden=(), table_rank1=True)
    plan = plan_of(api, tmp_path, W.embedding_from_spec(spec, "a", tail="none"))
    assert kinds(plan) == ["Embed"]
    s = plan["plan"]["steps"][0]
    assert s["pieces"] == [lookup(9, 1, 0, 0, 0), lookup(4, 1, 1, 1, 1), lookup(6, 1, 2, 2, 2), {"copy": 1, "src": 3, "out": 3}]
    assert "Unsqueeze:unsq1" in s["origin"].split("+")


def test_table_elements_per_model_are_capped(api, tmp_path):
    """32769 x 4096 zeros = 2^27 + 4096 elements (512 MiB + 16 KiB), written to the file piece by piece"""
    V, d = 32769, 4096
    raw = V * d * 4
    head = W._vi(1, V) + W._vi(1, d) + W._vi(2, W.FLOAT) + W._tag(9, 2) + W._varint(raw)
    tail = W._s(8, "table")
    nodes = W._ld(1, W.node("Gather", ["table", "x_cat"], ["e"], name="emb"))
    graph_head = nodes + W._s(2, "big") + W._tag(5, 2) + W._varint(len(head) + raw + len(tail)) + head
    graph_tail = tail + W._ld(11, W.value_info("x_cat", ["N", 1], W.INT64)) + W._ld(12, W.value_info("e", ["N", 1, d]))
    front = W._vi(1, 8) + W._s(2, "infera_amd") + W._tag(7, 2) + W._varint(len(graph_head) + raw + len(graph_tail))
    path = os.path.join(str(tmp_path), "big.onnx")
    chunk = bytes(1 << 24)
    with open(path, "wb") as f:
        f.write(front + graph_head)
        for _ in range(raw // len(chunk)):
            f.write(chunk)
        f.write(bytes(raw % len(chunk)))
        f.write(graph_tail + W._ld(8, W._s(1, "") + W._vi(2, 13)))
    with pytest.raises(api.InferaError) as e:
        api.load_model("big", path)
        api.unload_model("big")
    os.remove(path)
    assert str(e.value).endswith("ONNX error: node 'emb' (Gather): unsupported operator form: the model's Embed steps hold more than 2^27 table elements "
                                 "(134221824); 512 MiB is the cap"), str(e.value)


def test_graphs_without_a_lookup_keep_their_plans(api, tmp_path):
    """An integer input in front of a OneHotEncoder region, and a Gather(axis = 1) column pick behind a classifier, lower as before"""
    spec = W.prep_spec()
    assert "Embed" not in kinds(plan_of(api, tmp_path, W.prep_from_spec(spec)))
    nodes = [W.node("MatMul", ["X", "Wm"], ["h"]), W.node("Gather", ["h", "one"], ["Y"], [W.attr_i("axis", 1)], name="pick")]
    plan = plan_of(api, tmp_path, W.model("pick", nodes, [W.tensor("Wm", np.ones((3, 4), np.float32)), i64("one", [1])], [W.value_info("X", ["N", 3])], [W.value_info("Y", ["N", 1])]))
    assert kinds(plan) == ["Dense", "SliceCols"]


# ---- refusals, each in its own words --------------------------------------------------------------------------------------------------------
TABLE = np.zeros((5, 3), np.float32)


def lookup_model(table, idx_nodes=(), idx="x_cat", inputs=None, attrs=(), inits=()):
    nodes = list(idx_nodes) + [W.node("Gather", ["table", idx], ["e"], list(attrs), name="emb")]
    return W.model("m", nodes, [table] + list(inits), inputs or [W.value_info("x_cat", ["N", 1], W.INT64)], [W.value_info("e", ["N", 1, 3])])


def raw_table(dims, floats):
    """a TensorProto whose dims need not agree with its data"""
    return b"".join(W._vi(1, d) for d in dims) + W._vi(2, W.FLOAT) + W._ld(9, np.zeros(floats, "<f4").tobytes()) + W._s(8, "table")


FORM = r"ONNX error: node 'emb' \(Gather\): unsupported operator form: "
REFUSALS = {
    "float16 table": (lambda: lookup_model(W.tensor("table", TABLE.astype(np.float16))), FORM + "a table of type float16; only f32 tables are looked up"),
    "int64 table": (lambda: lookup_model(i64("table", np.zeros((5, 3)))), FORM + "a table of type int64; only f32 tables are looked up"),
    "int8 table": (lambda: lookup_model(W.tensor("table", np.zeros((5, 3), np.int8))), FORM + "a table of type int8; only f32 tables are looked up"),
    "rank 3": (lambda: lookup_model(W.tensor("table", np.zeros((5, 3, 2), np.float32))), FORM + r"a table of rank 3; only \[V, d\] and \[V\] tables"),
    "V = 0": (lambda: lookup_model(W.tensor("table", np.zeros((0, 3), np.float32))), FORM + r"an empty table \(V = 0, d = 3\)"),
    "d = 0": (lambda: lookup_model(W.tensor("table", np.zeros((3, 0), np.float32))), FORM + r"an empty table \(V = 3, d = 0\)"),
    "V > 2^24": (lambda: lookup_model(W.tensor("table", np.zeros(((1 << 24) + 1,), np.float32))), FORM + "a table of V = 16777217 rows, above the cap of 16777216"),
    "d > 4096": (lambda: lookup_model(W.tensor("table", np.zeros((1, 4097), np.float32))), FORM + "a table of d = 4097 columns, above the cap of 4096"),
    "1025 pieces": (lambda: lookup_model(W.tensor("table", TABLE), inputs=[W.value_info("x_cat", ["N", 1025], W.INT64)]), FORM + "1025 pieces, above the cap of 1024 per step"),
    "indices of rank 3": (lambda: lookup_model(W.tensor("table", TABLE), inputs=[W.value_info("x_cat", ["N", 2, 3], W.INT64)]),
                          FORM + r"indices of rank 3 \(graph input 'x_cat'\); only \[N\] and \[N, k\]"),
    "time-major indices": (lambda: lookup_model(W.tensor("table", TABLE), [W.node("Transpose", ["x_cat"], ["xt"], [W.attr_ints("perm", [1, 0])], name="tr")], idx="xt"),
                           FORM + "indices computed by Transpose 'tr'; only columns of a graph input"),
    "computed indices": (lambda: lookup_model(W.tensor("table", TABLE), [W.node("Relu", ["X"], ["r"], name="act"), W.node("Cast", ["r"], ["ri"], [W.attr_i("to", W.INT64)])],
                                              idx="ri", inputs=[W.value_info("X", ["N", 1])]), FORM + "indices computed by Relu 'act'; only columns of a graph input"),
    "scattered columns": (lambda: lookup_model(W.tensor("table", TABLE), [W.node("Gather", ["x_cat", "cols"], ["xc"], [W.attr_i("axis", 1)])], idx="xc",
                                               inputs=[W.value_info("x_cat", ["N", 4], W.INT64)], inits=[i64("cols", [2, 0])]), FORM + "index columns picked out of order"),
    "axis 1": (lambda: lookup_model(W.tensor("table", TABLE), attrs=[W.attr_i("axis", 1)]), FORM + r"axis = 1 of a constant table; a lookup takes whole rows \(axis = 0\)"),
    "data against dims": (lambda: lookup_model(raw_table((5, 3), 4)), "ONNX error: tensor 'table': element count does not match dims"),
    "V . d overflows": (lambda: lookup_model(raw_table((1 << 40, 1 << 40), 4)), "ONNX error: tensor 'table': element count does not match dims"),
    "offset beyond int64": (lambda: lookup_model(W.tensor("table", TABLE), [W.node("Add", ["x_cat", "o"], ["i1"])], idx="i1", inits=[i64("o", [(1 << 63) - 1])]),
                            FORM + r"an index offset beyond 2\^24"),
    "offsets that overflow together": (lambda: lookup_model(W.tensor("table", TABLE), [W.node("Add", ["x_cat", "o"], ["i1"]), W.node("Add", ["i1", "o"], ["i2"])], idx="i2",
                                                            inits=[i64("o", [(1 << 62) + 5])]), FORM + r"an index offset beyond 2\^24"),
    "negative offset beyond": (lambda: lookup_model(W.tensor("table", TABLE), [W.node("Add", ["o", "x_cat"], ["i1"])], idx="i1", inits=[i64("o", [-(1 << 24) - 1])]),
                               FORM + r"an index offset beyond 2\^24"),
    "offsets of the wrong length": (lambda: lookup_model(W.tensor("table", TABLE), [W.node("Add", ["x_cat", "o"], ["i1"])], idx="i1", inits=[i64("o", [1, 2, 3])],
                                                         inputs=[W.value_info("x_cat", ["N", 2], W.INT64)]), FORM + r"an offset tensor \[3\] added to 2 index columns; only a scalar, \[k\] or \[1, k\]"),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refusals(api, tmp_path, case):
    import re

    make, pattern = REFUSALS[case]
    msg = load_error(api, tmp_path, make())
    assert re.match(pattern, msg), msg


def test_output_row_beyond_the_cap_is_refused(api, tmp_path):
    """1 lookup + 1023 copies of a [N, 2^21 + 4096] input: 1024 pieces, more than 2^31 floats a row"""
    wide = (1 << 21) + 4096
    nodes = [W.node("Gather", ["X", "c0"], ["col"], [W.attr_i("axis", 1)]), W.node("Cast", ["col"], ["ci"], [W.attr_i("to", W.INT64)]), W.node("Gather", ["table", "ci"], ["e"], name="emb"),
             W.node("Concat", ["e"] + ["X"] * 1023, ["Y"], [W.attr_i("axis", 1)], name="join")]
    msg = load_error(api, tmp_path, W.model("m", nodes, [W.tensor("table", TABLE), i64("c0", 0)], [W.value_info("X", ["N", wide])], [W.value_info("Y", ["N", 3 + 1023 * wide])]))
    assert msg == "ONNX error: node 'emb' (Gather): unsupported operator form: an output row beyond 2^31 elements", msg


def test_wide_rows_leave_the_map_and_the_staging(api, tmp_path):
    """rows beyond 8192 output columns take the search over the pieces, a source row beyond the LDS tile is read where it lies: both load"""
    spec = W.embedding_spec(cards=(30,) * 40, dims=256, numeric=0, hidden=())
    s = plan_of(api, tmp_path, W.embedding_from_spec(spec, "c", tail="none"))["plan"]["steps"][0]
    assert (s["out_cols"], s["rows_per_tile"], s["staged"]) == (10240, 1, True)
    nodes = [W.node("Gather", ["X", "c0"], ["col"], [W.attr_i("axis", 1)]), W.node("Cast", ["col"], ["ci"], [W.attr_i("to", W.INT64)]), W.node("Gather", ["table", "ci"], ["Y"], name="emb")]
    blob = W.model("m", nodes, [W.tensor("table", TABLE), i64("c0", 9000)], [W.value_info("X", ["N", 9001])], [W.value_info("Y", ["N", 3])])
    s = plan_of(api, tmp_path, blob)["plan"]["steps"][0]
    assert (s["W"], s["staged"], s["pieces"]) == (9001, False, [lookup(5, 3, 9000, 0)])


# ---- the writer's references ----------------------------------------------------------------------------------------------------------------
def test_reference_is_table_of_idx(api):
    spec = W.embedding_spec(cards=(7, 11, 5), dims=(3, 4, 2), numeric=2, hidden=(4,))
    x_cat, x_num, x = W.embedding_inputs(spec, 9, seed=3)
    ref = W.embedding_reference(spec, x_cat, x_num, "a")
    want = np.concatenate([spec["tables"][0][x_cat[:, 0]], spec["tables"][1][x_cat[:, 1]], spec["tables"][2][x_cat[:, 2]], x_num], axis=1)
    assert np.array_equal(ref["features"], want) and ref["output"].dtype == np.float64 and ref["output"].shape == (9, 1)
    assert x.shape == (9, 5) and np.array_equal(x[:, :3], x_cat.astype(np.float32))
    sb = W.embedding_spec(cards=(7, 11), dims=4, numeric=0, hidden=())
    ids = np.array([[6, 0], [3.9, -0.5]])  # (values are truncated toward zero, then the column's offset is added)
    got = W.embedding_reference(sb, ids, None, "b", tail="none", flatten="window")["features"]
    assert got.shape == (2, 2, 4) and np.array_equal(got[:, 0], sb["tables"][0][[6, 3]]) and np.array_equal(got[:, 1], sb["tables"][1][[0, 0]])
    assert np.array_equal(W.embedding_lookup_reference(spec["tables"][0], [-7, -1]), spec["tables"][0][[0, 6]])  # ONNX's negative indices
    with pytest.raises(IndexError):
        W.embedding_lookup_reference(spec["tables"][0], [7])
    with pytest.raises(IndexError):
        W.embedding_lookup_reference(spec["tables"][0], [np.nan])
