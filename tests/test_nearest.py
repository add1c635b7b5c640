"""Distance models and feature-axis reductions at load time (no GPU): the plans the writer's graphs lower to, the switch to the
operator-by-operator plan, what keeps a graph from being the Nearest pattern, every rejection with its node, and the float64 references
against scikit-learn."""
from __future__ import annotations

import numpy as np
import pytest

from infera_amd import onnx_writer as W


@pytest.fixture(scope="module")
def api(built):
    from infera_amd import capi

    return capi


def _plan(api, tmp_path, name, blob, select=""):
    p = W.write(str(tmp_path / f"{name}.onnx"), blob)
    api.load_model(name, p + select)
    try:
        return api.get_plan(name)["plan"]
    finally:
        api.unload_model(name)


def kinds(plan):
    return [s["kind"] for s in plan["steps"]]


GENERIC = {"gemm": ["RowReduce", "PadCols", "Dense", "BinaryAct", "AffineChannel"], "matmul_mul": ["RowReduce", "PadCols", "Dense", "AffineChannel", "BinaryAct", "AffineChannel"],
           "cdist": ["RowReduce", "PadCols", "Dense", "BinaryAct", "AffineChannel"]}


@pytest.mark.parametrize("spelling", W.NEAREST_SPELLINGS)
def test_kmeans_plans(api, tmp_path, monkeypatch, spelling):
    spec = W.kmeans_spec(30, 100, seed=3)
    plan = _plan(api, tmp_path, "km", W.kmeans_from_spec(spec, spelling, "label"))
    assert kinds(plan) == ["Nearest", "NearestReduce"] and plan["output_shape"] == [-1]
    nn = plan["steps"][0]["nearest"]
    assert nn == {"F": 30, "M": 100, "k": 1, "outputs": "lists", "slices": 1, "slice_tile": [0, 4], "spelling": spelling, "centred": True}
    assert plan["steps"][1]["nearest"]["outputs"] == "label" and plan["flops_per_row"] == 2 * 30 * 100
    plan = _plan(api, tmp_path, "km_s", W.kmeans_from_spec(spec, spelling, "scores"))
    assert kinds(plan) == ["Nearest"] and plan["steps"][0]["nearest"]["outputs"] == "sqrt_d2" and plan["output_shape"] == [-1, 100]
    plan = _plan(api, tmp_path, "km_d", W.kmeans_from_spec(spec, spelling, "d2"))
    assert kinds(plan) == ["Nearest"] and plan["steps"][0]["nearest"]["outputs"] == "d2"
    if spelling != "cdist":
        assert kinds(_plan(api, tmp_path, "km_o", W.kmeans_from_spec(spec, spelling, "label", order="c2_first"))) == ["Nearest", "NearestReduce"]
    monkeypatch.setenv("INFERA_NEAREST", "0")
    plan = _plan(api, tmp_path, "km_g", W.kmeans_from_spec(spec, spelling, "label"))
    assert kinds(plan) == GENERIC[spelling] + ["ArgMin"], kinds(plan)
    assert kinds(_plan(api, tmp_path, "km_gs", W.kmeans_from_spec(spec, spelling, "scores")))[-1] in ("AffineChannel", "Unary")


def test_knn_search_plans_and_served_type(api, tmp_path):
    spec = W.kmeans_spec(128, 65536 // 16, seed=4)
    blob = W.knn_search_from_spec(spec, 10, "indices")
    plan = _plan(api, tmp_path, "knn", blob)
    assert kinds(plan) == ["Nearest", "NearestReduce"] and plan["output_shape"] == [-1, 10]
    assert plan["steps"][0]["nearest"]["k"] == 10 and plan["steps"][0]["nearest"]["slices"] == 16 and plan["steps"][1]["nearest"]["outputs"] == "indices"
    plan = _plan(api, tmp_path, "knn_d", blob, "#distances")
    assert kinds(plan) == ["Nearest", "NearestReduce"] and plan["steps"][1]["nearest"]["outputs"] == "sqrt_values"
    plan = _plan(api, tmp_path, "knn_g", W.knn_search_from_spec(spec, 10, "distances", "gemm"))
    assert kinds(plan) == ["Nearest", "NearestReduce", "Unary"] and plan["steps"][1]["nearest"]["outputs"] == "values"
    p = W.write(str(tmp_path / "knn_i.onnx"), blob)
    api.load_model("knn_i", p)
    try:
        assert "int64 output 'indices'" in api.get_model_info("knn_i")["output_served_as"]
    finally:
        api.unload_model("knn_i")


def test_not_the_pattern_lowers_generically(api, tmp_path):
    spec = W.kmeans_spec(8, 40, seed=5)
    c2 = (spec["centers"].astype(np.float64) ** 2).sum(1)
    ok = c2 * (1 + 4 * 2.0 ** -23)  # inside F 2^-23
    assert kinds(_plan(api, tmp_path, "c2_ok", W.kmeans_from_spec(spec, "gemm", "label", c2=ok)))[0] == "Nearest"
    off = c2.copy()
    off[7] *= 1 + 64 * 2.0 ** -23
    assert "Nearest" not in kinds(_plan(api, tmp_path, "c2_off", W.kmeans_from_spec(spec, "gemm", "label", c2=off)))
    plan = _plan(api, tmp_path, "two_readers", W.kmeans_from_spec(spec, "gemm", "label", extra_reader=True))
    assert kinds(plan) == ["RowReduce", "Dense", "BinaryAct", "AffineChannel", "ArgMin"]


READERS = [  # what stands between D2 and its consumer -> the plan (the pending distance value must never be read as a buffer)
    ("identity_out", [("Identity", [])], ["Nearest"], "d2"),
    ("sqrt_identity_out", [("Sqrt", []), ("Identity", [])], ["Nearest"], "sqrt_d2"),
    ("identity_argmin", [("Identity", []), ("ArgMin", [W.attr_i("axis", 1), W.attr_i("keepdims", 0)])], ["Nearest", "NearestReduce"], "lists"),
    ("flatten_relu", [("Flatten", []), ("Relu", [])], ["Nearest", "Unary"], "d2"),
    ("reshape_out", [("Reshape", [], np.array([0, -1], np.int64))], ["Nearest"], "d2"),
    ("sqrt_flatten_out", [("Sqrt", []), ("Flatten", [])], ["Nearest"], "sqrt_d2"),
    ("sqrt_reshape_neg", [("Sqrt", []), ("Reshape", [], np.array([0, -1], np.int64)), ("Neg", [])], ["Nearest", "Unary"], "sqrt_d2"),
    ("dropout_argmin", [("Dropout", []), ("ArgMin", [W.attr_i("axis", 1), W.attr_i("keepdims", 0)])], ["Nearest", "ArgMin"], "d2"),
]


@pytest.mark.parametrize("name,readers,want,outputs", READERS, ids=[r[0] for r in READERS])
@pytest.mark.parametrize("spelling", ["gemm", "cdist"])
def test_readers_of_the_distances(api, tmp_path, spelling, name, readers, want, outputs):
    spec = W.kmeans_spec(8, 40, seed=6)
    plan = _plan(api, tmp_path, name, W.distance_reader_graph(spec, readers, spelling))
    assert kinds(plan) == want, kinds(plan)
    assert plan["steps"][0]["nearest"]["outputs"] == outputs and plan["steps"][0]["in"] == 0
    for s in plan["steps"]:
        assert s["in"] >= 0 and s["out"] > 0, s


def test_reduce_zoo_plans(api, tmp_path):
    for axes_input in (False, True):
        blob, names = W.reduce_zoo(2, 5, axes_input=axes_input)
        for nm in names:
            plan = _plan(api, tmp_path, "zoo", blob, "#" + nm)
            want = ["RowReduce"] if nm[0] == "r" else ["RowReduce", "BinaryAct"] if nm[0] == "b" else ["ArgMin"] if nm == "argmin" else ["TopK"]
            assert kinds(plan) == want, nm
            if nm[0] == "r":
                assert plan["steps"][0]["op"] == nm[len("r_Reduce"):] and plan["steps"][0]["E"] == 5 and plan["output_shape"] == [-1, 1]
            if nm[0] == "b":
                assert plan["steps"][1]["row_scalar"] == ("left" if nm in ("b_Sub_l", "b_Div_l") else "right")
    blob, names = W.reduce_zoo(3, 5, T=3, keepdims=0)
    plan = _plan(api, tmp_path, "zoo3", blob, "#r_ReduceL2")
    assert kinds(plan) == ["RowReduce"] and plan["steps"][0]["T"] == 3 and plan["output_shape"] == [-1, 3]
    assert kinds(_plan(api, tmp_path, "zoo3b", W.reduce_zoo(3, 5, T=3)[0], "#b_Sub_l")) == ["RowReduce", "BinaryAct"]
    assert kinds(_plan(api, tmp_path, "ae", W.autoencoder()[0])) == ["Dense", "Dense", "BinaryAct", "BinaryAct", "RowReduce"]


def test_decomposed_layernorm_keeps_its_step(api, tmp_path):
    nodes, inits = [], []
    g, b = np.ones(16, np.float32), np.zeros(16, np.float32)
    W.layernorm_nodes(nodes, inits, "X", g, b, "Y", "ln", 1e-5, form="decomposed")
    blob = W.model("ln", nodes, inits, [W.value_info("X", ["N", 16])], [W.value_info("Y", ["N", 16])], opset=13)
    assert kinds(_plan(api, tmp_path, "ln", blob)) == ["LayerNorm"]


def _one(op, ins, outs, attrs=(), inits=(), dims=("N", 6), out_dims=("N", 1), out_type=W.FLOAT, opset=13, domain=""):
    nd = W.node(op, ins, outs, list(attrs), name="bad", domain=domain)
    return W.model("one", [nd], list(inits), [W.value_info("X", list(dims))], [W.value_info(outs[-1] if op == "TopK" else outs[0], list(out_dims), out_type)], opset=opset)


FORM = r"node 'bad' \((\w+)\): unsupported operator form: "
K = lambda v: [W.tensor("k", np.array([v], np.int64))]
REJECTS = [
    ("empty_axes", _one("ReduceSum", ["X"], ["Y"]), FORM + "empty axes"),
    ("noop", _one("ReduceSum", ["X", "ax"], ["Y"], [W.attr_i("noop_with_empty_axes", 1)], [W.tensor("ax", np.zeros(0, np.int64))]), FORM + "noop_with_empty_axes"),
    ("row_axis", _one("ReduceMax", ["X"], ["Y"], [W.attr_ints("axes", [0])]), FORM + "only the last axis"),
    ("two_axes", _one("ReduceL2", ["X"], ["Y"], [W.attr_ints("axes", [1, 2])], dims=("N", 3, 2)), FORM + "only the last axis"),
    ("middle_axis", _one("ReduceSumSquare", ["X"], ["Y"], [W.attr_ints("axes", [1])], dims=("N", 3, 2)), FORM + "only the last axis"),
    ("wide", _one("ReduceSum", ["X"], ["Y"], [W.attr_ints("axes", [1])], dims=("N", 65537)), FORM + "F = 65537 elements per reduced vector, above the cap of 65536"),
    ("argmin_last", _one("ArgMin", ["X"], ["Y"], [W.attr_i("axis", 1), W.attr_i("select_last_index", 1)], out_type=W.INT64), r"node 'bad' \(ArgMin\): select_last_index=1"),
    ("argmin_axis", _one("ArgMin", ["X"], ["Y"], [W.attr_i("axis", 0)], out_type=W.INT64), r"node 'bad' \(ArgMin\): only axis 1"),
    ("topk_big", _one("TopK", ["X", "k"], ["V", "I"], [], K(17), dims=("N", 40), out_dims=("N", 17), out_type=W.INT64), FORM + "k = 17 is outside 1 .. 16"),
    ("topk_over_m", _one("TopK", ["X", "k"], ["V", "I"], [], K(7), out_dims=("N", 7), out_type=W.INT64), FORM + "k = 7 is above the row length M = 6"),
    ("topk_axis", _one("TopK", ["X", "k"], ["V", "I"], [W.attr_i("axis", 0)], K(2), out_dims=("N", 2), out_type=W.INT64), FORM + "only the last axis"),
    ("topk_dyn", W.model("one", [W.node("Shape", ["X"], ["s"]), W.node("ReduceSum", ["X"], ["r"], [W.attr_ints("axes", [1]), W.attr_i("keepdims", 0)]),
                                 W.node("Cast", ["r"], ["kk"], [W.attr_i("to", W.INT64)]), W.node("TopK", ["X", "kk"], ["V", "I"], name="bad")], [],
                         [W.value_info("X", ["N", 6])], [W.value_info("I", ["N", 2], W.INT64)]), r"node 'bad' \(TopK\)"),
    ("cdist_metric", _one("CDist", ["X", "C"], ["Y"], [W.attr_s("metric", "cityblock")], [W.tensor("C", np.zeros((4, 6), np.float32))], out_dims=("N", 4),
                          domain=W.MS_DOMAIN), FORM + "metric 'cityblock'"),
    ("cdist_wide", _one("CDist", ["X", "C"], ["Y"], [], [W.tensor("C", np.zeros((2, 1025), np.float32))], dims=("N", 1025), out_dims=("N", 2), domain=W.MS_DOMAIN),
     FORM + "input width 1025 is above the cap of 1024"),
]


@pytest.mark.parametrize("name,blob,pattern", REJECTS, ids=[r[0] for r in REJECTS])
def test_rejections(api, tmp_path, name, blob, pattern):
    p = W.write(str(tmp_path / f"{name}.onnx"), blob)
    with pytest.raises(api.InferaError, match=pattern):
        api.load_model("bad_" + name, p)


def test_nearest_caps(api, tmp_path):
    """a KMeans graph over the width cap is rejected naming the node that closes the pattern"""
    spec = {"features": 1025, "centers": np.zeros((3, 1025), np.float32)}
    p = W.write(str(tmp_path / "wide.onnx"), W.kmeans_from_spec(spec, "gemm", "label"))
    with pytest.raises(api.InferaError, match=r"node 'add_c2' \(Add\): unsupported operator form: input width 1025 is above the cap of 1024"):
        api.load_model("bad_wide", p)


def test_references_agree_with_sklearn():
    cluster = pytest.importorskip("sklearn.cluster")
    from sklearn.datasets import make_blobs
    from sklearn.neighbors import NearestNeighbors

    x, _ = make_blobs(n_samples=400, n_features=5, centers=6, random_state=1)
    km = cluster.KMeans(6, n_init=2, random_state=0).fit(x[:300])
    spec = W.sklearn_kmeans_spec(km)
    ref = W.nearest_reference({"features": 5, "centers": km.cluster_centers_}, x[300:], 1)
    assert np.array_equal(ref["label"], km.predict(x[300:]))
    assert np.allclose(np.sqrt(ref["d2"]), km.transform(x[300:]), rtol=1e-9, atol=1e-9)
    assert spec["centers"].dtype == np.float32 and spec["features"] == 5
    nn = NearestNeighbors(n_neighbors=7).fit(x[:300])
    nspec = W.sklearn_neighbors_spec(nn)
    ref = W.nearest_reference({"features": 5, "centers": nn._fit_X}, x[300:], 7)
    dist, idx = nn.kneighbors(x[300:])
    assert np.array_equal(ref["indices"], idx) and np.allclose(np.sqrt(ref["values"]), dist, rtol=1e-9, atol=1e-9)
    assert nspec["n_neighbors"] == 7 and (ref["gap_out"] >= 0).all() and (ref["gap_in"] >= 0).all()
    assert (ref["mag"] >= ref["d2"] * (1 - 1e-12)).all()


def test_predict_without_gpu_fails(api, tmp_path):
    p = W.write(str(tmp_path / "km.onnx"), W.kmeans_from_spec(W.kmeans_spec(4, 3), "gemm"))
    api.load_model("km_nogpu", p)
    try:
        if api.device_count() > 0:  # (with a GPU the same call serves the labels)
            assert api.predict("km_nogpu", np.zeros((2, 4), np.float32)).shape[0] == 2
            return
        with pytest.raises(api.InferaError, match="HIP backend unavailable"):
            api.predict("km_nogpu", np.zeros((2, 4), np.float32))
    finally:
        api.unload_model("km_nogpu")
