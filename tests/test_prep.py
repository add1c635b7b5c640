"""ai.onnx.ml preprocessing regions at load time (no GPU): the plan of skl2onnx-shaped ColumnTransformer pipelines, integer inputs, ZipMap
output selection, every rejection (INTEGRATION.md section 2.6 "Preprocessing"), and a guard that graphs without a preprocessing region
plan exactly as before."""
from __future__ import annotations

import json
import os

import numpy as np
import pytest

from infera_amd import onnx_writer as W

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "plans_before_prep.json")


@pytest.fixture(scope="module")
def api(built):
    from infera_amd import capi

    return capi


def _load(api, tmp_path, name, blob, select=""):
    p = W.write(str(tmp_path / f"{name}.onnx"), blob)
    api.load_model(name, p + select)
    try:
        return api.get_plan(name), api.get_model_info(name)
    finally:
        api.unload_model(name)


def _kinds(plan):
    return [s["kind"] for s in plan["plan"]["steps"]]


def _prep(plan):
    p = [s for s in plan["plan"]["steps"] if s["kind"] == "Prep"]
    assert len(p) == 1, plan["plan"]["steps"]
    return p[0]


SPEC = W.prep_spec()  # the reference shape: 6 numeric, 8 categorical (100 categories), 2 ordinal (20 keys) -> F' = 108


def _tree(seed=5, kind="classifier"):
    return W.tree_ensemble_spec(features=W.prep_width(SPEC), trees=10, depth=4, kind=kind, seed=seed)


def test_reference_shape_width():
    assert SPEC["features"] == 16 and W.prep_width(SPEC) == 108


def test_pipeline_tree_plan(api, tmp_path):
    plan, info = _load(api, tmp_path, "pt", W.prep_from_spec(SPEC, head=W.tree_head(_tree())))
    assert _kinds(plan) == ["Prep", "TreeEnsemble", "TreeReduce"]
    p = _prep(plan)
    assert p["F_in"] == 16 and p["F"] == 108 and p["onehot_cols"] == 100 and p["lookup_cols"] == 2 and p["strict"] is False
    assert p["rows_per_tile"] == 512 and p["in"] == 0
    for op in ("ArrayFeatureExtractor:num_afe", "Imputer:num_imputer", "Scaler:num_scaler", "OneHotEncoder:cat0_onehot", "Cast:cat0_cast",
               "Reshape:cat0_reshape", "LabelEncoder:ord1_encoder", "Concat:concat"):
        assert op in p["origin"].split("+"), (op, p["origin"])
    assert info["input_shape"] == [-1, 16] and info["output_shape"] == [-1]


@pytest.mark.parametrize("layout", [dict(after_onehot="Flatten"), dict(after_onehot="Squeeze"), dict(cast=False), dict(concat_axis=-1)],
                         ids=["flatten", "squeeze", "nocast", "axis-1"])
def test_exporter_variants(api, tmp_path, layout):
    plan, _ = _load(api, tmp_path, "pv", W.prep_from_spec(SPEC, head=W.tree_head(_tree()), **layout))
    assert _kinds(plan) == ["Prep", "TreeEnsemble", "TreeReduce"]
    assert _prep(plan)["F"] == 108


def test_svm_and_linear_heads_and_prep_only(api, tmp_path):
    Fp = W.prep_width(SPEC)
    svm = W.svm_spec(features=Fp, n_sv=64, classes=3, seed=3)
    plan, _ = _load(api, tmp_path, "ps", W.prep_from_spec(SPEC, head=W.svm_head(svm)))
    assert _kinds(plan) == ["Prep", "SvmKernel", "SvmReduce"]
    rng = np.random.default_rng(0)
    lin = W.linear_head(rng.normal(0, 0.1, (3, Fp)), rng.normal(0, 0.1, 3), [0, 1, 2])
    plan, _ = _load(api, tmp_path, "pl", W.prep_from_spec(SPEC, head=lin), "#probabilities")
    assert _kinds(plan)[0] == "Prep" and "Dense" in _kinds(plan)
    plan, info = _load(api, tmp_path, "po", W.prep_from_spec(SPEC))
    assert _kinds(plan) == ["Prep"] and info["output_shape"] == [-1, 108]


def _int_model(with_float: bool, elem=W.INT64):
    nodes = [W.node("OneHotEncoder", ["C"], ["oh"], [W.attr_ints("cats_int64s", [1, 2, 5])], name="oh", domain=W.ML_DOMAIN),
             W.node("Reshape", ["oh", "shp"], ["ohf"], name="rs")]
    inits = [W.tensor("shp", np.asarray([-1, 6], dtype=np.int64))]
    inputs = [W.value_info("C", ["N", 2], elem)]
    out = "ohf"
    if with_float:
        nodes.append(W.node("Concat", ["Xf", "ohf"], ["all"], [W.attr_i("axis", 1)], name="cc"))
        inputs = [W.value_info("Xf", ["N", 3])] + inputs
        out = "all"
    return W.model("ints", nodes, inits, inputs, [W.value_info(out, ["N", 9 if with_float else 6])], ml_opset=3)


def test_integer_inputs(api, tmp_path):
    plan, info = _load(api, tmp_path, "i1", _int_model(False))
    assert _kinds(plan) == ["Prep"] and _prep(plan)["F_in"] == 2 and info["output_shape"] == [-1, 6]
    plan, info = _load(api, tmp_path, "i2", _int_model(True, W.INT32 if hasattr(W, "INT32") else 6))
    assert _kinds(plan) == ["Prep"] and _prep(plan)["F_in"] == 5 and info["input_shape"] == [-1, 5] and info["output_shape"] == [-1, 9]
    # an int64 input alone in front of a tree ensemble: truncated by a Prep step
    tree = W.tree_ensemble_spec(features=4, trees=3, depth=3, seed=2)
    blob = W.tree_ensemble_from_spec(tree)
    blob = blob.replace(W.value_info("X", ["N", 4]), W.value_info("X", ["N", 4], W.INT64))
    plan, _ = _load(api, tmp_path, "i3", blob)
    assert _kinds(plan) == ["Prep", "TreeEnsemble", "TreeReduce"]


def test_zipmap_output(api, tmp_path):
    tree = _tree(kind="classifier")
    blob = W.prep_from_spec(SPEC, head=W.tree_head(tree), zipmap=True)
    plan, info = _load(api, tmp_path, "zm", blob, "#output_probability")
    assert _kinds(plan) == ["Prep", "TreeEnsemble", "TreeReduce"] and info["output_shape"] == [-1, 3]
    assert info["output_served_as"] == ("f32 [rows, classes] probabilities read by the graph's ZipMap output 'output_probability', "
                                        "one column per class in classlabels order")
    plan, info = _load(api, tmp_path, "zl", blob)  # the label: the dead ZipMap branch is ignored
    assert info["output_shape"] == [-1] and "int64" in info["output_served_as"]


def test_non_contiguous_afe_alone(api, tmp_path):
    nodes = [W.node("ArrayFeatureExtractor", ["X", "ix"], ["Y"], name="afe", domain=W.ML_DOMAIN)]
    inits = [W.tensor("ix", np.asarray([3, 0, 3, 1], dtype=np.int64))]
    blob = W.model("afe", nodes, inits, [W.value_info("X", ["N", 5])], [W.value_info("Y", ["N", 4])], ml_opset=1)
    plan, _ = _load(api, tmp_path, "afe", blob)
    assert _kinds(plan) == ["Prep"] and _prep(plan)["F"] == 4


def test_strict_onehot_plan(api, tmp_path):
    plan, _ = _load(api, tmp_path, "st", W.prep_from_spec(W.prep_spec(strict=True)))
    assert _prep(plan)["strict"] is True


# ---- rejections ------------------------------------------------------------------------------------------------------------------

def _one(op, attrs, x_type=W.FLOAT, width=2, idx=None):
    nodes, inits, x = [], [], "X"
    if idx is not None:
        inits.append(W.tensor("ix", np.asarray(idx, dtype=np.int64)))
        nodes.append(W.node("ArrayFeatureExtractor", ["X", "ix"], ["Xp"], name="afe", domain=W.ML_DOMAIN))
        x = "Xp"
    if op:
        nodes.append(W.node(op, [x], ["Y"], attrs, name="bad", domain=W.ML_DOMAIN))
    else:
        nodes.append(W.node("Identity", [x], ["Y"], name="bad"))
    return W.model("bad", nodes, inits, [W.value_info("X", ["N", width], x_type)], [W.value_info("Y", ["N", 1])], ml_opset=3)


def _cap_one_hot(n_nodes, per):
    nodes, parts = [], []
    for i in range(n_nodes):
        nodes.append(W.node("OneHotEncoder", ["X"], [f"o{i}"], [W.attr_ints("cats_int64s", range(per))], name=f"oh{i}", domain=W.ML_DOMAIN))
        nodes.append(W.node("Flatten", [f"o{i}"], [f"f{i}"], [W.attr_i("axis", 1)]))
        parts.append(f"f{i}")
    nodes.append(W.node("Concat", parts, ["Y"], [W.attr_i("axis", 1)]))
    return W.model("cap", nodes, [], [W.value_info("X", ["N", 1])], [W.value_info("Y", ["N", n_nodes * per])], ml_opset=3)


REJECT = [
    ("cats_strings", _one("OneHotEncoder", [W.attr_strings("cats_strings", ["a", "b"])]), r"\(OneHotEncoder\): cats_strings: string categories"),
    ("no_cats", _one("OneHotEncoder", []), r"needs cats_int64s"),
    ("big_cat", _one("OneHotEncoder", [W.attr_ints("cats_int64s", [1, (1 << 24) + 1])]), r"beyond 2\^24"),
    ("le_strings", _one("LabelEncoder", [W.attr_strings("keys_strings", ["a"]), W.attr_floats("values_floats", [1.0])]), r"keys_strings: string keys"),
    ("le_values_strings", _one("LabelEncoder", [W.attr_ints("keys_int64s", [1]), W.attr_strings("values_strings", ["a"])]), r"values_strings"),
    ("le_dup", _one("LabelEncoder", [W.attr_floats("keys_floats", [1.0, -0.0, 0.0]), W.attr_floats("values_floats", [1, 2, 3])]),
     r"duplicate key 0"),
    ("le_len", _one("LabelEncoder", [W.attr_ints("keys_int64s", [1, 2, 3]), W.attr_floats("values_floats", [1, 2])]),
     r"keys and values differ in length \(3 vs 2\)"),
    ("le_big_value", _one("LabelEncoder", [W.attr_ints("keys_int64s", [1]), W.attr_ints("values_int64s", [1 << 25])]), r"beyond 2\^24"),
    ("imputer_len", _one("Imputer", [W.attr_floats("imputed_value_floats", [1, 2, 3])], width=2),
     r"imputed_value_floats holds 3 values, expected 1 or 2"),
    ("imputer_none", _one("Imputer", []), r"exactly one of imputed_value_floats"),
    ("afe_range", _one("", [], idx=[0, 5]), r"column index 5 out of range for 2 columns"),
    ("afe_negative", _one("", [], idx=[1, -1]), r"negative column index -1"),
    ("fv_dims", W.model("fv", [W.node("FeatureVectorizer", ["X", "X"], ["Y"], [W.attr_ints("inputdimensions", [2, 3])], name="fv",
                                      domain=W.ML_DOMAIN)], [], [W.value_info("X", ["N", 2])], [W.value_info("Y", ["N", 4])], ml_opset=1),
     r"inputdimensions\[1\] = 3 but input 'X' has 2 columns"),
    ("string_input", _one("Binarizer", [], x_type=8), r"input 'X' is not f32, int64 or int32"),
    ("double_input", _one("Binarizer", [], x_type=11), r"input 'X' is not f32, int64 or int32"),
    ("cap_source", _one("", [], width=5000, idx=[0, 2]), r"reads 5000 source columns; at most 4096"),
    ("cap_out", _one("OneHotEncoder", [W.attr_ints("cats_int64s", range(5000))], width=2), r"one-hot columns; a preprocessing step writes at most 8192"),
    ("cap_cats", _cap_one_hot(9, 8000), r"more than 65536 one-hot categories in all"),
]


@pytest.mark.parametrize("name,blob,pat", REJECT, ids=[r[0] for r in REJECT])
def test_rejections(api, tmp_path, name, blob, pat):
    p = W.write(str(tmp_path / f"{name}.onnx"), blob)
    with pytest.raises(api.InferaError, match=pat):
        api.load_model("rej_" + name, p)


def test_cap_label_encoder_keys(api, tmp_path):
    keys = np.arange(600_000, dtype=np.int64)
    nodes = [W.node("LabelEncoder", ["X"], [f"l{i}"], [W.attr_ints("keys_int64s", keys), W.attr_floats("values_floats", keys % 7)],
                    name=f"le{i}", domain=W.ML_DOMAIN) for i in range(2)]
    nodes.append(W.node("Concat", ["l0", "l1"], ["Y"], [W.attr_i("axis", 1)]))
    blob = W.model("capk", nodes, [], [W.value_info("X", ["N", 1])], [W.value_info("Y", ["N", 2])], ml_opset=3)
    p = W.write(str(tmp_path / "capk.onnx"), blob)
    with pytest.raises(api.InferaError, match=r"more than 1048576 LabelEncoder keys in all"):
        api.load_model("capk", p)


# ---- regression guard --------------------------------------------------------------------------------------------------------------

def _writer_models():
    yield "linear_dyn", W.linear_dyn()
    yield "mlp", W.mlp()
    yield "mlp_softmax", W.mlp(final_softmax=True)
    yield "logreg_softmax", W.logreg_softmax()
    yield "identity", W.identity()
    yield "unary_zoo", W.unary_zoo()
    yield "exporter_reshape", W.exporter_reshape()
    yield "concat_heads", W.concat_heads()
    yield "se_net", W.se_net()
    yield "zoo_ops_net", W.zoo_ops_net()[0]
    yield "mobilenet_v2", W.mobilenet_v2()
    yield "resnet18", W.resnet18()
    for kind in ("classifier", "regressor"):
        for out in ("label", "scores"):
            yield f"sklearn_pipeline_{kind}_{out}", W.sklearn_pipeline(kind=kind, output=out)
    yield "sklearn_pipeline_norm", W.sklearn_pipeline(normalizer="L2", output="scores")
    yield "tree_regressor", W.tree_ensemble(trees=8, depth=4, seed=3)
    yield "tree_classifier", W.tree_ensemble(kind="classifier", trees=8, depth=4, post="SOFTMAX", seed=4)
    yield "tree_classifier_probs", W.tree_ensemble(kind="classifier", trees=8, depth=4, output="probabilities", seed=4)
    yield "tree_scaler", W.tree_ensemble(scaler=([0.5] * 30, [2.0] * 30), trees=8, depth=4, seed=5)
    yield "svm_classifier", W.svm(n_sv=64, seed=6)
    yield "svm_classifier_probs", W.svm(n_sv=64, probabilities=True, output="probabilities", seed=6)
    yield "svm_regressor", W.svm(kind="regressor", n_sv=64, seed=7)
    yield "svm_scaler", W.svm(scaler=([0.5] * 30, [2.0] * 30), n_sv=64, seed=8)


def test_existing_models_plan_unchanged(api, tmp_path):
    """The plans recorded (tests/golden/plans_before_prep.json) from the commit before preprocessing regions existed."""
    with open(GOLDEN) as fh:
        want = json.load(fh)
    got = {}
    for name, blob in _writer_models():
        p = W.write(str(tmp_path / f"{name}.onnx"), blob)
        api.load_model("g_" + name, p)
        try:
            got[name] = api.get_plan("g_" + name)["plan"]
        finally:
            api.unload_model("g_" + name)
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], name
