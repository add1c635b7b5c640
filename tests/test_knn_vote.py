"""k-NN classifiers and regressors at load time (no GPU): every graph form the writer restates plans as Nearest -> NearestVote, what keeps
the search outputs' NearestReduce steps, every rejection with its node, the refusals that stay as they were without the matcher, and the
float64 reference against scikit-learn (INTEGRATION.md section 2.6 "The k-NN vote")."""
from __future__ import annotations

import numpy as np
import pytest

from infera_amd import onnx_writer as W
from tests import knn_vote_ref as R


@pytest.fixture(scope="module")
def api(built):
    from infera_amd import capi

    return capi


_n = [0]


def _load(api, tmp_path, blob, select=""):
    _n[0] += 1
    name = f"vote{_n[0]}"
    p = W.write(str(tmp_path / f"{name}.onnx"), blob)
    api.load_model(name, p + select)
    try:
        return api.get_plan(name)["plan"], api.get_model_info(name)
    finally:
        api.unload_model(name)


def kinds(plan):
    return [s["kind"] for s in plan["steps"]]


SPEC = W.kmeans_spec(6, 40, seed=1)
Y = np.arange(40) % 3
CLASSES = [3, 7, 8]  # (not evenly spaced)

CLASSIFIER_FORMS = [
    dict(), dict(weights="distance"), dict(output="probabilities"), dict(output="probabilities", weights="distance"),
    dict(spelling="gemm"), dict(spelling="gemm", weights="distance"), dict(spelling="matmul_mul"), dict(spelling="matmul_mul", weights="distance", output="probabilities"),
    dict(lookup="gather"), dict(lookup="gather", weights="distance", output="probabilities"), dict(keepdims=0), dict(keepdims=0, output="probabilities"),
    dict(keepdims=0, join="transpose"), dict(keepdims=0, join="transpose", weights="distance", output="probabilities"), dict(reshape="k1"), dict(reshape="k", lookup="gather"),
    dict(cast=True), dict(reciprocal="div", weights="distance"), dict(final="none"), dict(final="reshape_cast"), dict(final="cast", lookup="gather"),
]


@pytest.mark.parametrize("form", CLASSIFIER_FORMS, ids=lambda f: "-".join(f"{k}={v}" for k, v in f.items()) or "default")
def test_classifier_forms_plan_as_one_vote(api, tmp_path, form):
    plan, info = _load(api, tmp_path, W.knn_classifier_from_spec(SPEC, Y, CLASSES, 5, **form))
    assert kinds(plan) == ["Nearest", "NearestVote"], kinds(plan)
    near, vote = plan["steps"]
    assert near["nearest"]["outputs"] == "lists" and near["nearest"]["k"] == 5 and vote["in"] == near["out"]
    proba = form.get("output") == "probabilities"
    assert vote["k"] == 5 and vote["classes"] == 3 and vote["weights"] == form.get("weights", "uniform") and vote["outputs"] == ("probabilities" if proba else "label")
    assert vote["rooted"] is (form.get("spelling", "cdist") == "cdist" or form.get("weights") == "distance")  # (a gemm spelling roots the values only where they are read)
    assert plan["output_shape"] == ([-1, 3] if proba else [-1])
    if proba:
        assert "output_served_as" not in info
    else:
        assert "int64 output 'label'" in info["output_served_as"]


REGRESSOR_FORMS = [dict(), dict(weights="distance"), dict(keepdims=1), dict(keepdims=1, weights="distance"), dict(final="none"), dict(final="none", keepdims=1, weights="distance"),
                   dict(spelling="gemm", weights="distance"), dict(spelling="matmul_mul"), dict(lookup="gather"), dict(lookup="gather", weights="distance", reciprocal="div"),
                   dict(reshape="k1")]


@pytest.mark.parametrize("integer", [False, True], ids=["f32", "int64"])
@pytest.mark.parametrize("form", REGRESSOR_FORMS, ids=lambda f: "-".join(f"{k}={v}" for k, v in f.items()) or "default")
def test_regressor_forms_plan_as_one_vote(api, tmp_path, form, integer):
    t = np.arange(40) - 7 if integer else (np.arange(40) / 3).astype(np.float32)
    plan, _ = _load(api, tmp_path, W.knn_regressor_from_spec(SPEC, t, 5, **form))
    assert kinds(plan) == ["Nearest", "NearestVote"], kinds(plan)
    vote = plan["steps"][1]
    assert vote["k"] == 5 and vote["classes"] == 0 and vote["weights"] == form.get("weights", "uniform") and vote["outputs"] == "value"
    assert plan["output_shape"] == ([-1] if form.get("final") == "none" and not form.get("keepdims") else [-1, 1])
    assert plan["flops_per_row"] == 2 * 6 * 40 + 2 * 5


def test_search_outputs_keep_their_steps(api, tmp_path):
    """Indices / Values that something else reads too get their NearestReduce steps as without the vote"""
    blob = W.knn_classifier_from_spec(SPEC, Y, CLASSES, 5, also=("indices", "distances"))
    assert kinds(_load(api, tmp_path, blob)[0]) == ["Nearest", "NearestVote"]  # (declared, not served: nothing reads them)
    plan, info = _load(api, tmp_path, blob, "#indices")
    assert kinds(plan) == ["Nearest", "NearestReduce"] and plan["steps"][1]["nearest"]["outputs"] == "indices" and "int64 output 'indices'" in info["output_served_as"]
    assert kinds(_load(api, tmp_path, blob, "#distances")[0]) == ["Nearest", "NearestReduce"]
    # a reader beside the vote: with a gemm spelling Sqrt(values) is a graph output AND feeds the weights, so the values are written
    blob = W.knn_classifier_from_spec(SPEC, Y, CLASSES, 5, spelling="gemm", weights="distance", also=("distances",))
    plan, _ = _load(api, tmp_path, blob)
    assert kinds(plan) == ["Nearest", "NearestReduce", "Unary", "NearestVote"], kinds(plan)
    assert plan["steps"][1]["nearest"]["outputs"] == "values" and plan["steps"][3]["in"] == plan["steps"][0]["out"] and plan["steps"][3]["rooted"] is True


def test_zipmap_serves_the_probabilities(api, tmp_path):
    plan, info = _load(api, tmp_path, W.knn_classifier_from_spec(SPEC, Y, CLASSES, 5, output="probabilities", zipmap=True))
    assert kinds(plan) == ["Nearest", "NearestVote"] and plan["output_shape"] == [-1, 3] and plan["steps"][1]["outputs"] == "probabilities"
    assert "ZipMap output 'output_probability'" in info["output_served_as"]


def test_label_has_no_class_cap_and_many_slices(api, tmp_path):
    spec = W.kmeans_spec(4, 600, seed=2)
    plan, _ = _load(api, tmp_path, W.knn_classifier_from_spec(spec, np.arange(600) % 257, list(range(257)), 16))
    assert kinds(plan) == ["Nearest", "NearestVote"] and plan["steps"][1]["classes"] == 257 and plan["steps"][1]["slices"] == plan["steps"][0]["nearest"]["slices"] >= 2
    plan, _ = _load(api, tmp_path, W.knn_classifier_from_spec(spec, np.arange(600) % 256, list(range(256)), 16, output="probabilities"))
    assert plan["steps"][1]["classes"] == 256 and plan["output_shape"] == [-1, 256]


FORM = r"node '%s' \(%s\): unsupported operator form: "
REJECTS = [
    ("table_short", lambda: W.knn_classifier_from_spec(SPEC, Y[:39], CLASSES, 5), FORM % ("lookup", "ArrayFeatureExtractor") + "its table holds 39 entries for the M = 40 reference vectors"),
    ("table_short_gather", lambda: W.knn_regressor_from_spec(SPEC, np.zeros(41, np.float32), 5, lookup="gather"), FORM % ("lookup", "Gather") + "its table holds 41 entries for the M = 40"),
    ("class_index", lambda: W.knn_classifier_from_spec(SPEC, np.where(np.arange(40) == 17, 3, Y), CLASSES, 5),
     FORM % ("lookup", "ArrayFeatureExtractor") + r"class index 3 of reference vector 17 is outside 0 \.\. 2"),
    ("class_index_negative", lambda: W.knn_classifier_from_spec(SPEC, np.where(np.arange(40) == 0, -1, Y), CLASSES, 5), FORM % ("lookup", "ArrayFeatureExtractor") + "class index -1 of reference vector 0"),
    ("equal_order", lambda: W.knn_classifier_from_spec(SPEC, Y, CLASSES, 5, equal_values=[0, 2, 1]),
     FORM % ("equal1", "Equal") + r"the class branches must compare with 0 \.\. 2 in Concat order; branch 1 compares with 2"),
    ("eps_zero", lambda: W.knn_classifier_from_spec(SPEC, Y, CLASSES, 5, weights="distance", eps=0.0), FORM % ("clamp", "Max") + "the bound of the distance weights must be one positive finite constant"),
    ("eps_negative", lambda: W.knn_regressor_from_spec(SPEC, Y.astype(np.float32), 5, weights="distance", eps=-1e-6), FORM % ("clamp", "Max") + "the bound of the distance weights"),
    ("eps_inf", lambda: W.knn_classifier_from_spec(SPEC, Y, CLASSES, 5, weights="distance", eps=np.inf, output="probabilities"), FORM % ("clamp", "Max") + "the bound of the distance weights"),
    ("eps_nan", lambda: W.knn_classifier_from_spec(SPEC, Y, CLASSES, 5, weights="distance", eps=np.nan), FORM % ("clamp", "Max") + "the bound of the distance weights"),
    ("one_class", lambda: W.knn_classifier_from_spec(SPEC, np.zeros(40, np.int64), [4], 5), FORM % ("concat", "Concat") + "C = 1 class: a vote needs at least 2"),
    ("proba_cap", lambda: W.knn_classifier_from_spec(SPEC, Y, list(range(257)), 5, output="probabilities"),
     FORM % ("concat", "Concat") + "C = 257 classes is above the cap of 256 for the probabilities"),
    ("class_value", lambda: W.knn_classifier_from_spec(SPEC, Y, [0, 1, 2 ** 24 + 1], 5), FORM % ("class_lookup", "ArrayFeatureExtractor") + r"class value 16777217 is beyond 2\^24"),
    ("class_value_negative", lambda: W.knn_classifier_from_spec(SPEC, Y, [-2 ** 25, 1, 2], 5, lookup="gather"), FORM % ("class_lookup", "Gather") + r"class value -33554432 is beyond 2\^24"),
    ("multi_output", lambda: W.knn_regressor_from_spec(SPEC, np.zeros((40, 2), np.float32), 5),
     FORM % ("lookup", "ArrayFeatureExtractor") + r"its table \[40,2\] holds several targets per reference vector: multi-output"),
    ("k_17", lambda: W.knn_classifier_from_spec(SPEC, Y, CLASSES, 17), FORM % ("topk", "TopK") + r"k = 17 neighbours of a k-NN vote is outside 1 \.\. 16"),
    ("k_over_m", lambda: W.knn_regressor_from_spec(W.kmeans_spec(6, 4, seed=1), np.zeros(4, np.float32), 5), FORM % ("topk", "TopK") + r"k = 5 neighbours of a k-NN vote is outside 1 \.\. 4"),
    ("k_zero", lambda: W.knn_classifier_from_spec(SPEC, Y, CLASSES, 0, output="probabilities"), FORM % ("topk", "TopK") + r"k = 0 neighbours of a k-NN vote is outside 1 \.\. 16"),
]


@pytest.mark.parametrize("name,blob,pattern", REJECTS, ids=[r[0] for r in REJECTS])
def test_rejections(api, tmp_path, name, blob, pattern):
    p = W.write(str(tmp_path / f"{name}.onnx"), blob())
    with pytest.raises(api.InferaError, match=pattern):
        api.load_model("bad_vote_" + name, p)


# the messages of the commit before the vote, recorded there from these very graphs
PARENT_AFE = r"node 'lookup' \(ArrayFeatureExtractor\): class table must be evenly spaced \(label = a \+ b \* index\)"
PARENT_GATHER = r"node 'lookup' \(Gather\): unsupported operator form: a table of type int64; only f32 tables are looked up \(float16, integer and quantised tables are not\)"


@pytest.mark.parametrize("lookup,message", [("afe", PARENT_AFE), ("gather", PARENT_GATHER)])
@pytest.mark.parametrize("reader", ["knn_all", "knn_lab", "knn_wei"])
def test_outside_reader_is_refused_as_before(api, tmp_path, reader, lookup, message):
    """an intermediate that is a graph output too: not the pattern, so the load fails at the node and with the text it failed with before"""
    p = W.write(str(tmp_path / "extra.onnx"), W.knn_classifier_from_spec(SPEC, Y, CLASSES, 5, weights="distance", lookup=lookup, extra_reader=reader))
    with pytest.raises(api.InferaError, match=message):
        api.load_model("bad_vote_reader", p)


def test_operator_by_operator_switch_has_no_vote(api, tmp_path, monkeypatch):
    """INFERA_NEAREST=0: no plan for the vote (Equal stays unsupported); the load is refused as before"""
    monkeypatch.setenv("INFERA_NEAREST", "0")
    p = W.write(str(tmp_path / "generic.onnx"), W.knn_classifier_from_spec(SPEC, Y, CLASSES, 5))
    with pytest.raises(api.InferaError, match=PARENT_AFE):
        api.load_model("bad_vote_generic", p)
    p = W.write(str(tmp_path / "generic_g.onnx"), W.knn_classifier_from_spec(SPEC, Y, CLASSES, 5, lookup="gather"))
    with pytest.raises(api.InferaError, match=PARENT_GATHER):
        api.load_model("bad_vote_generic_g", p)


def test_evenly_spaced_rule_stays_elsewhere(api, tmp_path):
    """ArrayFeatureExtractor(class table, ArgMax) outside a vote still wants an evenly spaced table"""
    rng = np.random.default_rng(0)
    nodes = [W.node("MatMul", ["X", "w"], ["s"], name="scores"), W.node("ArgMax", ["s"], ["a"], [W.attr_i("axis", 1), W.attr_i("keepdims", 0)], name="argmax"),
             W.node("ArrayFeatureExtractor", ["classes", "a"], ["label"], name="class_lookup", domain=W.ML_DOMAIN)]
    inits = [W.tensor("w", rng.standard_normal((6, 3)).astype(np.float32)), W.tensor("classes", np.array(CLASSES, np.int64))]
    blob = W.model("afe", nodes, inits, [W.value_info("X", ["N", 6])], [W.value_info("label", ["N"], W.INT64)], ml_opset=1)
    p = W.write(str(tmp_path / "afe.onnx"), blob)
    with pytest.raises(api.InferaError, match=r"node 'class_lookup' \(ArrayFeatureExtractor\): class table must be evenly spaced"):
        api.load_model("bad_vote_afe", p)


# ---- the float64 reference against scikit-learn ----------------------------------------------------------------------------------

GENERIC = [(30, 600, 11, 5), (7, 100, 12, 16), (128, 1000, 13, 10)]  # F, M, seed, k: the generic inputs of tests/test_knn_vote_gpu.py


def generic_case(F, M, seed, k, C=4):
    spec = W.kmeans_spec(F, M, seed)
    x = np.random.default_rng(seed + 100).standard_normal((257, F)).astype(np.float32)
    rng = np.random.default_rng(seed + 200)
    return spec, x, rng.integers(0, C, M), rng.integers(-64, 65, M)


@pytest.mark.parametrize("F,M,seed,k", GENERIC)
def test_reference_agrees_with_sklearn(F, M, seed, k):
    nb = pytest.importorskip("sklearn.neighbors")
    spec, x, y, t = generic_case(F, M, seed, k)
    ref = W.nearest_reference(spec, x, k)
    classes = np.array([3, 7, 8, 20])
    c64, x64 = spec["centers"].astype(np.float64), x.astype(np.float64)  # (scikit-learn computes float32 inputs in float32)
    assert (np.sqrt(ref["values"]) > 1e-3).all()  # (no zero distance: scikit-learn treats those apart)
    for weights in ("uniform", "distance"):
        want = R.vote_reference(ref["indices"], np.sqrt(ref["values"]), y=y, target=t, C=4, weights=weights)
        clf = nb.KNeighborsClassifier(k, weights=weights, algorithm="brute").fit(c64, classes[y])
        assert np.allclose(clf.predict_proba(x64), want["proba"], rtol=1e-9, atol=0)
        assert np.array_equal(clf.predict(x64), classes[want["label"]])
        reg = nb.KNeighborsRegressor(k, weights=weights, algorithm="brute").fit(c64, t)
        assert np.allclose(reg.predict(x64), want["value"], rtol=1e-9, atol=1e-12)
        assert (np.abs(want["value"]) <= want["mag"] * (1 + 1e-12)).all()


def test_tied_vote_goes_to_the_lower_class():
    nb = pytest.importorskip("sklearn.neighbors")
    c = np.array([[0.0], [1.0], [10.0], [11.5]], np.float32)
    y = np.array([2, 1, 0, 2])
    x = np.array([[0.4], [10.5]], np.float32)  # neighbours (0, 1): classes 2 and 1 tie; (2, 3): classes 0 and 2 tie
    ref = W.nearest_reference({"features": 1, "centers": c}, x, 2)
    assert ref["indices"].tolist() == [[0, 1], [2, 3]]
    want = R.vote_reference(ref["indices"], np.sqrt(ref["values"]), y=y, C=3)
    assert want["label"].tolist() == [1, 0] and want["proba"].tolist() == [[0, 0.5, 0.5], [0.5, 0, 0.5]]
    assert R.vote_f32(ref["indices"], ref["values"], y=y, C=3)["label"].tolist() == [1, 0]
    assert nb.KNeighborsClassifier(2, algorithm="brute").fit(c, y).predict(x).tolist() == [1, 0]


def test_first_max_rule_on_nan():
    """the ArgMax step's rule, which a NaN row's label follows: element 0 starts the scan and a NaN never compares greater"""
    nan = np.nan
    assert R.first_max(np.array([[nan, 1.0, 2.0], [0.0, nan, nan], [1.0, nan, 3.0], [0.0, 0.0, 0.0]])).tolist() == [0, 0, 2, 0]


@pytest.mark.parametrize("case,excluded", list(zip(GENERIC, (0, 0, 1))))
def test_excluded_share_of_the_generic_inputs(case, excluded):
    """from the reference alone: the rows tests/test_knn_vote_gpu.py leaves out because their (k + 1)-th neighbour is within twice the distance
    bound of the k-th (0 %, 0 % and 0.4 % of the 257 rows)"""
    F, M, seed, k = case
    spec, x, _, _ = generic_case(F, M, seed, k)
    ex = excluded_rows(spec, x, k)
    assert int(ex.sum()) == excluded and ex.mean() <= 0.01


def excluded_rows(spec, x, k):
    ref = W.nearest_reference(spec, x, k)
    tol = R.tol_of(ref, spec["features"])
    near = np.argsort(ref["d2"], 1, kind="stable")[:, :k + 1]
    bound = np.take_along_axis(tol, near, 1).max(1)  # (the file's convention: the largest bound among the k + 1 nearest)
    return ref["gap_out"] < 2 * bound
