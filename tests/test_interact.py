"""Feature interactions without a GPU: what the loader recognises as the Interact step -- DLRM's T . T^T read whole, through Gather(axis = 1)
or through TorchScript's advanced-index sequence, and the FM bi-interaction term -- the plans it makes of them, the pass-through of DLRM's
cat([x, Zflat], 1), and what it refuses (INTEGRATION.md 2.6 "Feature interactions").  Every plan test fails on a loader without the step:
it refuses the MatMul of two activations and the ReduceSum over the middle axis."""
import os

import numpy as np
import pytest

from infera_amd import onnx_writer as W


@pytest.fixture(scope="module")
def api(built):
    from infera_amd import capi

    return capi


def plan_of(api, tmp_path, blob, name="ia"):
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


def kinds(plan):
    return [s["kind"] for s in plan["plan"]["steps"]]


def the_step(plan):
    steps = [s for s in plan["plan"]["steps"] if s["kind"] == "Interact"]
    assert len(steps) == 1, kinds(plan)
    return steps[0]


K, D = 8, 2
TABLE = np.arange(11 * D, dtype=np.float32).reshape(11, D)
FRONT = {"embed": ["Embed"], "reshape": [], "concat": ["SliceCols"] * K + ["CopyCols"] * K}


# ---- dot --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["embed", "reshape", "concat"])
@pytest.mark.parametrize("form", ["matrix", "flat", "gather", "index", "index_folded"])
def test_dot_plans(api, tmp_path, form, source):
    sel = W.interact_triangle(K)
    plan = plan_of(api, tmp_path, W.interact_dot_model(K, D, form, sel, source, TABLE))
    assert kinds(plan) == FRONT[source] + ["Interact"]
    s = the_step(plan)
    whole = form in ("matrix", "flat")
    P = K * K if whole else len(sel)
    assert (s["mode"], s["k"], s["d"], s["P"], s["out_cols"], s["whole"], s["pass_through"], s["tile"]) == ("dot", K, D, P, P, whole, [], 16)
    assert s["selection"] == (list(range(K * K)) if whole else sel.tolist()) and s["selection_out"] == 0
    assert s["bytes_per_row"] == 4 * (K * D + P)
    assert plan["plan"]["output_shape"] == ([-1, K, K] if form == "matrix" else [-1, P])
    assert plan["plan"]["flops_per_row"] == 2 * K * K * D
    names = s["origin"].split("+")
    assert names[:2] == ["Transpose:tr", "MatMul:dot"]
    if not whole:
        # the [N, k, k] matrix is never a buffer: everything the plan holds per row is T's sources, T and the P products
        assert "Gather:pairs" in names
        assert plan["scratch_floats_per_row"] < K * K, plan["scratch_floats_per_row"]
    if form == "index":  # the Shape sub-graphs of the exporter's sequence belong to the step
        for nm in ("Shape:zshape", "Gather:dim2", "Mul:idx_mul", "Add:idx_add", "Concat:final_shape", "Transpose:idx_back", "Reshape:idx_final"):
            assert nm in names, s["origin"]


@pytest.mark.parametrize("k,tile", [(2, 16), (16, 16), (17, 32), (32, 32), (33, 64), (64, 64)])
def test_tile_follows_k(api, tmp_path, k, tile):
    s = the_step(plan_of(api, tmp_path, W.interact_dot_model(k, 3, "gather", [0, -1, k * k - 1, 0])))
    assert (s["tile"], s["P"], s["selection"]) == (tile, 4, [0, k * k - 1, k * k - 1, 0])  # negative indices count from the end


def test_reshape_spelling_of_the_flattening(api, tmp_path):
    s = the_step(plan_of(api, tmp_path, W.interact_dot_model(K, D, "gather", [3, 1], flatten="reshape")))
    assert s["selection"] == [3, 1] and "Reshape:zflat" in s["origin"]


# ---- fm ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("square", ["mul", "pow"])
@pytest.mark.parametrize("h_side", ["right", "left"])
@pytest.mark.parametrize("sum_last", [False, True])
def test_fm_plans(api, tmp_path, square, h_side, sum_last):
    for source in ("embed", "reshape", "concat"):
        plan = plan_of(api, tmp_path, W.interact_fm_model(K, D, source, TABLE, square=square, h=0.5, h_side=h_side, sum_last=sum_last))
        assert kinds(plan) == FRONT[source] + ["Interact"]
        s = the_step(plan)
        assert (s["mode"], s["k"], s["d"], s["P"], s["h"], s["sum_last"], s["h_after_sum"]) == ("fm", K, D, 0, 0.5, sum_last, False)
        assert s["out_cols"] == (1 if sum_last else D) and plan["plan"]["output_shape"] == [-1, 1 if sum_last else D]
        sq = "Mul" if square == "mul" else "Pow"
        want = ["ReduceSum:fsum", f"{sq}:sq_sum", f"{sq}:sq", "ReduceSum:sum_sq", "Sub:diff", "Mul:half"] + (["ReduceSum:total"] if sum_last else [])
        assert s["origin"].split("+")[: len(want)] == want


def test_fm_spellings(api, tmp_path):
    """no h; keepdims = 1 on the field sums ([N, 1, d]); axes as an attribute (opset 11); the multiply behind the last-axis sum; a rank-1 result"""
    s = the_step(plan_of(api, tmp_path, W.interact_fm_model(K, D)))
    assert (s["h"], s["sum_last"], s["out_cols"]) == (None, False, D)
    plan = plan_of(api, tmp_path, W.interact_fm_model(K, D, keepdims=1, h=2.0))
    assert the_step(plan)["h"] == 2.0 and plan["plan"]["output_shape"] == [-1, 1, D]
    plan = plan_of(api, tmp_path, W.interact_fm_model(K, D, keepdims=1, sum_last=True, axes_input=False, opset=11))
    assert the_step(plan)["sum_last"] and plan["plan"]["output_shape"] == [-1, 1, 1]
    s = the_step(plan_of(api, tmp_path, W.interact_fm_model(K, D, h=0.5, sum_last=True, h_after=True)))
    assert (s["h"], s["sum_last"], s["h_after_sum"]) == (0.5, True, True)
    plan = plan_of(api, tmp_path, W.interact_fm_model(K, D, sum_last=True, last_keepdims=0))
    assert the_step(plan)["sum_last"] and plan["plan"]["output_shape"] == [-1]


# ---- whole models ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["gather", "index", "index_folded"])
def test_small_dlrm(api, tmp_path, form):
    """bottom MLP, Embed (the bottom MLP's result is a gap one CopyCols fills), Interact with x passed through, top MLP: the second Concat
    is part of the step and copies nothing"""
    spec = W.dlrm_spec(cards=(7, 11, 5), d=4, numeric=3, bottom=(8,), top=(8,))
    plan = plan_of(api, tmp_path, W.dlrm_from_spec(spec, form=form))
    assert kinds(plan) == ["SliceCols", "Dense", "Dense", "Embed", "CopyCols", "Interact", "Dense", "Dense"]
    s = the_step(plan)
    assert (s["mode"], s["k"], s["d"], s["P"], s["out_cols"]) == ("dot", 4, 4, 6, 10)
    assert s["pass_through"] == [{"src": 0, "len": 4, "out": 0}] and s["selection_out"] == 4 and s["selection"] == [4, 8, 9, 12, 13, 14]
    assert s["origin"].endswith("+Concat:cat_r") and s["bytes_per_row"] == 4 * (16 + 10)
    embed = plan["plan"]["steps"][3]
    assert s["in"] == embed["out"] and embed["pieces"][0] == {"gap": 4, "out": 0}
    top = plan["plan"]["steps"][6]
    assert (top["in"], top["K"]) == (s["out"], 10)
    assert plan["plan"]["output_shape"] == [-1, 1]


def test_dlrm_concat_that_is_no_pass_through_keeps_its_copies(api, tmp_path):
    """cat([Zsel, other], 1) with `other` not an input of the Concat that built T: the selection is the step, the Concat copies as before"""
    nodes, inits, T, inputs, _ = W.interact_window_nodes(K, D, "reshape")
    zsel, _ = W.interact_dot_nodes(nodes, inits, T, K, "gather", [1, 2, 3])
    nodes.append(W.node("Relu", ["X"], ["other"], name="other"))
    nodes.append(W.node("Concat", [zsel, "other"], ["Y"], [W.attr_i("axis", 1)], name="join"))
    plan = plan_of(api, tmp_path, W.model("nopass", nodes, inits, inputs, [W.value_info("Y", ["N", 3 + K * D])]))
    assert kinds(plan) == ["Interact", "Unary", "CopyCols", "CopyCols"]
    assert the_step(plan)["pass_through"] == [] and the_step(plan)["out_cols"] == 3


def test_small_deepfm(api, tmp_path):
    spec = W.deepfm_spec(cards=(7, 11, 5, 3), d=4, hidden=(8,))
    plan = plan_of(api, tmp_path, W.deepfm_from_spec(spec))
    assert kinds(plan) == ["Embed", "Embed", "RowReduce", "Interact", "Dense", "Dense", "BinaryAct", "BinaryAct"]
    s = the_step(plan)
    assert (s["mode"], s["k"], s["d"], s["h"], s["sum_last"], s["h_after_sum"], s["out_cols"]) == ("fm", 4, 4, 0.5, True, True, 1)
    assert s["in"] == plan["plan"]["steps"][0]["out"] and plan["plan"]["steps"][0]["window"] == [4, 4]
    assert plan["plan"]["steps"][4]["in"] == s["in"]  # the deep MLP reads the same window


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_caps(api, tmp_path):
    msg = load_error(api, tmp_path, W.interact_dot_model(65, 2, "matrix"))
    assert "node 'dot' (MatMul)" in msg and "k = 65 fields, above the cap of 64" in msg
    msg = load_error(api, tmp_path, W.interact_dot_model(4, 257, "matrix"))
    assert "node 'dot' (MatMul)" in msg and "d = 257 values per field, above the cap of 256" in msg
    msg = load_error(api, tmp_path, W.interact_dot_model(4, 2, "gather", np.zeros(4097, np.int64)))
    assert "node 'pairs' (Gather)" in msg and "P = 4097 selected products, above the cap of 4096" in msg
    msg = load_error(api, tmp_path, W.interact_dot_model(4, 2, "index_folded", np.zeros(4097, np.int64)))
    assert "node 'pairs' (Gather)" in msg and "P = 4097" in msg
    msg = load_error(api, tmp_path, W.interact_fm_model(65, 2))
    assert "node 'diff' (Sub)" in msg and "k = 65 fields" in msg
    msg = load_error(api, tmp_path, W.interact_fm_model(4, 257))
    assert "node 'diff' (Sub)" in msg and "d = 257 values per field" in msg
    # at the caps everything loads
    assert the_step(plan_of(api, tmp_path, W.interact_dot_model(64, 256, "gather", np.zeros(4096, np.int64))))["P"] == 4096


@pytest.mark.parametrize("bad", [16, -17, 1 << 40])
def test_index_out_of_range(api, tmp_path, bad):
    msg = load_error(api, tmp_path, W.interact_dot_model(4, 2, "gather", [0, bad, 3]))
    assert "node 'pairs' (Gather)" in msg and f"index {bad} is outside [-16, 16)" in msg
    if bad > 0:
        msg = load_error(api, tmp_path, W.interact_dot_model(4, 2, "index_folded", [0, bad, 3]))
        assert "node 'pairs' (Gather)" in msg and f"index {bad} is outside [-16, 16)" in msg


# what the loader said of these products before this step, word for word: the matcher passes them by and the attention matcher words the
# refusal as it always did (a rank-3 Transpose in front of the product reads as nn.MultiheadAttention's time-major export)
TIME_MAJOR = ("unsupported operator form: PyTorch nn.MultiheadAttention's time-major export (heads folded into the row axis, [T, N*h, dh]) is not "
              "supported yet; export batch-first projections with the head split Reshape [N,T,h,dh] -> Transpose(0,2,1,3)")
GENERIC = ("unsupported operator form: MatMul of two activations outside a recognised self-attention pattern (Reshape [N,T,h,dh] -> "
           "Transpose(0,2,1,3), Q K^T, scale, constant mask, Softmax(-1), P V, Transpose(0,2,1,3) -> Reshape [N,T,E]); the right operand must "
           "otherwise be a constant weight matrix")


def test_product_of_two_different_values(api, tmp_path):
    nodes, inits, T, inputs, _ = W.interact_window_nodes(K, D, "reshape")
    nodes.append(W.node("Relu", [T], ["T2"], name="other"))
    W.interact_dot_nodes(nodes, inits, T, K, "matrix", right="T2")
    msg = load_error(api, tmp_path, W.model("two", nodes, inits, inputs, [W.value_info("Z", ["N", K, K])]))
    assert msg == "ONNX error: node 'dot' (MatMul): " + TIME_MAJOR


def test_other_transpose_perm(api, tmp_path):
    """perm (0,1,2) gives [N,k,d] x [N,k,d]; perm (1,0,2) a time-major operand: neither is T^T, both keep the refusal"""
    for perm in ((0, 1, 2), (1, 0, 2), (2, 1, 0)):
        nodes, inits, T, inputs, _ = W.interact_window_nodes(K, D, "reshape")
        W.interact_dot_nodes(nodes, inits, T, K, "matrix", perm=perm)
        msg = load_error(api, tmp_path, W.model("perm", nodes, inits, inputs, [W.value_info("Z", ["N", K, K])]))
        assert msg == "ONNX error: node 'dot' (MatMul): " + TIME_MAJOR, (perm, msg)


def test_rows_mixing_product_stays_refused(api, tmp_path):
    """[N, F] x [F, N]: one value on both sides, but the product mixes rows"""
    nodes = [W.node("Transpose", ["X"], ["Xt"], [W.attr_ints("perm", [1, 0])], name="tr"), W.node("MatMul", ["X", "Xt"], ["Y"], name="dot")]
    msg = load_error(api, tmp_path, W.model("mix", nodes, [], [W.value_info("X", ["N", 6])], [W.value_info("Y", ["N", "N"])]))
    assert msg == "ONNX error: node 'dot' (MatMul): " + GENERIC


def test_runtime_product_that_is_no_gram_matrix_keeps_its_message(api, tmp_path):
    nodes = [W.node("Relu", ["X"], ["A"]), W.node("Sigmoid", ["X"], ["B"]), W.node("MatMul", ["A", "B"], ["Y"], name="ab")]
    msg = load_error(api, tmp_path, W.model("ab", nodes, [], [W.value_info("X", ["N", 4, 4])], [W.value_info("Y", ["N", 4, 4])]))
    assert msg == "ONNX error: node 'ab' (MatMul): " + GENERIC


def test_fm_inner_value_with_a_second_reader(api, tmp_path):
    """the field sum S is also a graph output's source: the pattern is not matched and ReduceSum over axis 1 keeps its refusal"""
    for inner in ("S", "SS", "Q", "QS"):
        nodes, inits, T, inputs, _ = W.interact_window_nodes(K, D, "reshape")
        cur, dims = W.interact_fm_nodes(nodes, inits, T, D)
        nodes.append(W.node("Relu", [inner], ["side"], name="side"))
        nodes.append(W.node("Add" if inner in ("S", "SS", "QS") else "ReduceSum", [cur, "side"] if inner != "Q" else ["side", "fsum_axes"], ["Y"], [] if inner != "Q" else [W.attr_i("keepdims", 0)], name="join"))
        if inner == "Q":
            nodes.append(W.node("Add", [cur, "Y"], ["Y2"], name="join2"))
        msg = load_error(api, tmp_path, W.model("second", nodes, inits, inputs, [W.value_info("Y2" if inner == "Q" else "Y", ["N", D])]))
        assert "(ReduceSum)" in msg and "only the last axis" in msg, (inner, msg)


@pytest.mark.parametrize("front", ["input", "dense"])
@pytest.mark.parametrize("kw", [dict(keepdims=1), dict(keepdims=1, h=0.5), dict(keepdims=1, square="pow", h=0.5, h_side="left", sum_last=True)])
def test_fm_over_scalar_fields_plans_as_before(api, tmp_path, front, kw):
    """(sum x)^2 - sum x^2 on a RANK-2 activation [N, k]: axis 1 is the last axis there, the single operators always served it, and they
    still do -- the pattern is claimed before shapes are known and given up where T is no window"""
    inits = []
    if front == "input":
        nodes, x, inputs = [], "X", [W.value_info("X", ["N", 6])]
    else:
        inits.append(W.tensor("Wf", np.arange(35, dtype=np.float32).reshape(7, 5) / 35))
        nodes, x, inputs = [W.node("MatMul", ["X", "Wf"], ["H"], name="fc")], "H", [W.value_info("X", ["N", 7])]
    cur, _ = W.interact_fm_nodes(nodes, inits, x, 1, **kw)
    plan = plan_of(api, tmp_path, W.model("scalar_fm", nodes, inits, inputs, [W.value_info(cur, ["N", 1])]))
    got = kinds(plan)
    assert "Interact" not in got and got.count("RowReduce") == (3 if kw.get("sum_last") else 2), got
    assert [k_ for k_ in got if k_ not in ("Dense", "RowReduce", "BinaryAct", "BinaryConst", "AffineChannel", "Unary")] == [], got
    assert plan["plan"]["output_shape"] == [-1, 1]
    if front == "input" and kw == dict(keepdims=1):
        assert got == ["RowReduce", "BinaryAct", "BinaryAct", "RowReduce", "BinaryAct"]


def _index_model_with_front_reshapes(k, d, targets):
    """the folded advanced-index form with Reshape nodes (constant targets) in place of its Flatten(2)"""
    nodes, inits, T, inputs, _ = W.interact_window_nodes(k, d, "reshape")
    cur, dims = W.interact_dot_nodes(nodes, inits, T, k, "index_folded", W.interact_triangle(k))
    at = [i for i, n in enumerate(nodes) if b"idx_flat" in n]
    assert len(at) == 1
    chain, src = [], "Zt"
    for j, tgt in enumerate(targets):
        inits.append(W.tensor(f"front_shape{j}", np.asarray(tgt, dtype=np.int64)))
        dst = "Zf" if j + 1 == len(targets) else f"Zf{j}"
        chain.append(W.node("Reshape", [src, f"front_shape{j}"], [dst], name=f"front{j}"))
        src = dst
    nodes[at[0] : at[0] + 1] = chain
    return W.model("front", nodes, inits, inputs, [W.value_info(cur, ["N"] + dims)])


def test_advanced_index_reshapes_in_front_of_the_gather(api, tmp_path):
    """[k, k, N] may only become [k * k, N] there: a target that would read it as [N, k * k] gives other values than the model's"""
    k, d = 4, 2
    for targets in ([[k * k, -1]], [[-1, k * k][::-1]], [[k * k, -1], [k * k, -1]]):
        assert the_step(plan_of(api, tmp_path, _index_model_with_front_reshapes(k, d, targets)))["P"] == 6
    for targets, node in (([[-1, k * k]], "front0"), ([[k * k, -1], [-1, k * k]], "front1"), ([[k * k, -1], [4, -1]], "front1"), ([[8, -1]], "front0")):
        msg = load_error(api, tmp_path, _index_model_with_front_reshapes(k, d, targets))
        assert f"node '{node}' (Reshape)" in msg and "only the flattening of [k, k, N] to [k * k, N] is matched" in msg, (targets, msg)


def test_time_major_window(api, tmp_path):
    """T = Transpose(1,0,2) of the window: its row axis is axis 1"""
    for mode in ("dot", "fm"):
        nodes, inits, T, inputs, _ = W.interact_window_nodes(K, D, "reshape")
        nodes.append(W.node("Transpose", [T], ["Ttm"], [W.attr_ints("perm", [1, 0, 2])], name="tm"))
        if mode == "dot":
            W.interact_dot_nodes(nodes, inits, "Ttm", K, "matrix")
            out = W.value_info("Z", [K, "N", "N"])
        else:
            cur, _ = W.interact_fm_nodes(nodes, inits, "Ttm", D)
            out = W.value_info(cur, [K, D])
        msg = load_error(api, tmp_path, W.model("tm", nodes, inits, inputs, [out]))
        assert ("node 'dot' (MatMul)" if mode == "dot" else "node 'diff' (Sub)") in msg and "time-major" in msg and "rows first" in msg


def test_einsum_stays_refused(api, tmp_path):
    nodes, inits, T, inputs, _ = W.interact_window_nodes(K, D, "reshape")
    nodes.append(W.node("Einsum", [T, T], ["Y"], [W.attr_s("equation", "nid,njd->nij")], name="es"))
    msg = load_error(api, tmp_path, W.model("es", nodes, inits, inputs, [W.value_info("Y", ["N", K, K])]))
    assert "Einsum" in msg


def test_graphs_without_the_patterns_plan_as_before(api, tmp_path):
    assert kinds(plan_of(api, tmp_path, W.mlp((8, 16, 4)))) in (["Dense", "Dense"], ["Dense", "Unary", "Dense"])
    spec = W.embedding_spec(cards=(7, 11, 5), dims=(3, 4, 2), numeric=2, hidden=(16, 8))
    assert kinds(plan_of(api, tmp_path, W.embedding_from_spec(spec, "a"))) == ["Embed", "Dense", "Dense", "Dense"]
