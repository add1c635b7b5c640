"""ai.onnx.ml TreeEnsembleRegressor / TreeEnsembleClassifier at load time (no GPU): the plan a seeded ensemble lowers to, output
selection, and every form that is rejected with its reason."""
from __future__ import annotations

import numpy as np
import pytest

from infera_amd import onnx_writer as W


@pytest.fixture(scope="module")
def api(built):
    from infera_amd import capi

    return capi


def _load(api, tmp_path, name, blob, select=""):
    p = W.write(str(tmp_path / f"{name}.onnx"), blob)
    api.load_model(name, p + select)
    try:
        return api.get_plan(name)
    finally:
        api.unload_model(name)


def _tree_steps(plan):
    steps = plan["plan"]["steps"]
    walk = [s for s in steps if s["kind"] == "TreeEnsemble"]
    assert len(walk) == 1, steps
    return walk[0], steps


def test_full_trees_plan(api, tmp_path):
    spec = W.tree_ensemble_spec(features=30, trees=100, depth=6, seed=3)
    plan = _load(api, tmp_path, "full", W.tree_ensemble_from_spec(spec))
    walk, steps = _tree_steps(plan)
    assert walk["trees"] == 100 and walk["nodes"] == 100 * 127 and walk["max_depth"] == 6 and walk["E"] == 1
    assert walk["slices"] == 13 and walk["aggregate"] == "SUM" and walk["output"] == "scores"
    assert [s["kind"] for s in steps] == ["TreeEnsemble", "TreeReduce"]
    assert plan["plan"]["input_shape"] == [-1, 30] and plan["plan"]["output_shape"] == [-1, 1]


def test_ragged_multi_target_plan(api, tmp_path):
    spec = W.tree_ensemble_spec(features=8, trees=5, depth=22, ragged=True, targets=3, aggregate="AVERAGE", modes=W.TREE_MODES,
                                missing=True, base_values=True, seed=4)
    plan = _load(api, tmp_path, "ragged", W.tree_ensemble_from_spec(spec))
    walk, _ = _tree_steps(plan)
    assert walk["trees"] == 5 and walk["nodes"] == len(spec["nodes_treeids"]) and walk["max_depth"] == 22
    assert walk["E"] == 3 and walk["walk_width"] == 3 and walk["aggregate"] == "AVERAGE" and walk["slices"] == 1
    assert plan["plan"]["output_shape"] == [-1, 3]


def test_classifier_label_and_scores_selection(api, tmp_path):
    spec = W.tree_ensemble_spec(features=12, trees=20, depth=5, kind="classifier", labels=[3, 7, 42], post="SOFTMAX", seed=5)
    blob = W.tree_ensemble_from_spec(spec)
    plan = _load(api, tmp_path, "cls", blob)
    walk, steps = _tree_steps(plan)
    assert walk["E"] == 3 and walk["output"] == "label" and plan["plan"]["output_shape"] == [-1]
    assert "Softmax" not in [s["kind"] for s in steps]  # the label is taken before post_transform
    plan = _load(api, tmp_path, "cls_scores", blob, "#probabilities")
    walk, steps = _tree_steps(plan)
    assert walk["output"] == "scores" and plan["plan"]["output_shape"] == [-1, 3]
    assert [s["kind"] for s in steps] == ["TreeEnsemble", "TreeReduce", "Softmax"]


def test_binary_forms_plan(api, tmp_path):
    for binary, post in (("signed", "LOGISTIC"), ("positive", "NONE")):
        spec = W.tree_ensemble_spec(features=6, trees=9, depth=4, kind="classifier", binary=binary, post=post, base_values=True, seed=6)
        plan = _load(api, tmp_path, "bin_" + binary, W.tree_ensemble_from_spec(spec), "#probabilities")
        walk, steps = _tree_steps(plan)
        assert walk["E"] == 2 and walk["walk_width"] == 1 and walk["output"] == "binary_scores"
        assert plan["plan"]["output_shape"] == [-1, 2]
        plan = _load(api, tmp_path, "binl_" + binary, W.tree_ensemble_from_spec(spec))
        assert _tree_steps(plan)[0]["output"] == "binary_label"


def test_as_tensor_and_scaler_pipeline_load(api, tmp_path):
    spec = W.tree_ensemble_spec(features=10, trees=4, depth=5, as_tensor=True, modes=W.TREE_MODES, base_values=True, seed=8)
    plan = _load(api, tmp_path, "tensor", W.tree_ensemble_from_spec(spec, scaler=([0.5] * 10, [2.0] * 10)))
    walk, steps = _tree_steps(plan)
    assert steps[0]["kind"] != "TreeEnsemble"  # the Scaler runs first: its rounding is not folded into thresholds
    assert walk["nodes"] == 4 * 63


def test_threshold_conversion():
    """The f32 thresholds the loader derives from doubles (host/trees.cpp tree_threshold_f32), restated here."""
    def conv(d, direction):
        f = np.float32(d)
        if direction == 0 and float(f) > d:
            f = np.nextafter(f, np.float32(-np.inf))
        if direction == 1 and float(f) < d:
            f = np.nextafter(f, np.float32(np.inf))
        return f
    rng = np.random.default_rng(1)
    xs = rng.uniform(-2, 2, 2000).astype(np.float32)
    for d in rng.uniform(-2, 2, 50):
        for direction, op in ((0, np.less_equal), (1, np.less)):
            t = conv(d, direction)
            assert np.array_equal(op(xs, t), op(xs.astype(np.float64), d))


def _reject(api, tmp_path, name, attrs, pattern, F=4, op="TreeEnsembleRegressor", in_dims=None):
    outs = ["label", "scores"] if op == "TreeEnsembleClassifier" else ["Y"]
    nd = W.node(op, ["X"], outs, attrs, domain=W.ML_DOMAIN)
    out_vi = W.value_info(outs[0], ["N"] if op == "TreeEnsembleClassifier" else ["N", 1], W.INT64 if op == "TreeEnsembleClassifier" else W.FLOAT)
    blob = W.model(name, [nd], [], [W.value_info("X", in_dims or ["N", F])], [out_vi], ml_opset=1)
    p = W.write(str(tmp_path / f"{name}.onnx"), blob)
    with pytest.raises(api.InferaError, match=pattern):
        api.load_model("bad_" + name, p)


def _stump(**over):
    """One tree: node 0 (x[f] <= 0.5) -> leaves 1 / 2, as attribute dicts; `over` replaces arrays."""
    a = {"nodes_treeids": [0, 0, 0], "nodes_nodeids": [0, 1, 2], "nodes_featureids": [1, 0, 0],
         "nodes_modes": ["BRANCH_LEQ", "LEAF", "LEAF"], "nodes_values": [0.5, 0, 0], "nodes_truenodeids": [1, 0, 0],
         "nodes_falsenodeids": [2, 0, 0], "target_treeids": [0, 0], "target_nodeids": [1, 2], "target_ids": [0, 0],
         "target_weights": [1.0, 2.0]}
    a.update(over)
    return a


def _attrs(a):
    out = []
    for k, v in a.items():
        if k == "nodes_modes":
            out.append(W.attr_strings(k, v))
        elif k in ("nodes_values", "target_weights", "class_weights", "base_values"):
            out.append(W.attr_floats(k, v))
        elif isinstance(v, str):
            out.append(W.attr_s(k, v))
        elif isinstance(v, int):
            out.append(W.attr_i(k, v))
        else:
            out.append(W.attr_ints(k, v))
    return out


def test_stump_loads(api, tmp_path):
    p = W.write(str(tmp_path / "stump.onnx"), W.model("stump", [W.node("TreeEnsembleRegressor", ["X"], ["Y"], _attrs(_stump()), domain=W.ML_DOMAIN)],
                                                      [], [W.value_info("X", ["N", 4])], [W.value_info("Y", ["N", 1])], ml_opset=1))
    api.load_model("stump", p)
    walk, _ = _tree_steps(api.get_plan("stump"))
    api.unload_model("stump")
    assert (walk["trees"], walk["nodes"], walk["max_depth"]) == (1, 3, 1)


REJECTS = [
    ("cycle", _stump(nodes_modes=["BRANCH_LEQ", "BRANCH_LEQ", "LEAF"], nodes_truenodeids=[1, 0, 0], nodes_falsenodeids=[2, 2, 0]),
     r"more than one branch|cycle"),
    ("cycle2", _stump(nodes_treeids=[0, 0, 0, 1, 1], nodes_nodeids=[0, 1, 2, 0, 1], nodes_featureids=[1, 0, 0, 0, 0],
                      nodes_modes=["BRANCH_LEQ", "LEAF", "LEAF", "BRANCH_LT", "BRANCH_LT"], nodes_values=[0.5, 0, 0, 0, 0],
                      nodes_truenodeids=[1, 0, 0, 1, 0], nodes_falsenodeids=[2, 0, 0, 1, 0]), r"more than one branch|cycle|no root"),
    ("nochild", _stump(nodes_falsenodeids=[7, 0, 0]), r"names child 7, which does not exist in its tree"),
    ("dup", _stump(nodes_nodeids=[0, 1, 1]), r"duplicate node 1 of tree 0"),
    ("feature", _stump(nodes_featureids=[4, 0, 0]), r"feature id 4 is not below the input width 4"),
    ("mode", _stump(nodes_modes=["BRANCH_FOO", "LEAF", "LEAF"]), r"unknown node mode 'BRANCH_FOO'"),
    ("lengths", _stump(nodes_values=[0.5, 0]), r"attribute arrays of different lengths: nodes_values"),
    ("leaflengths", _stump(target_ids=[0]), r"attribute arrays of different lengths"),
    ("targets", _stump(n_targets=2000), r"E = 2000 outputs, above the cap of 1024"),
    ("minmax", _stump(aggregate_function="MAX"), r"aggregate_function MAX"),
    ("probit", _stump(post_transform="PROBIT"), r"post_transform PROBIT"),
    ("softmax_zero", _stump(post_transform="SOFTMAX_ZERO"), r"post_transform SOFTMAX_ZERO"),
    ("notleaf", _stump(target_nodeids=[0, 2]), r"which is not a leaf"),
    ("empty", {"nodes_treeids": []}, r"TreeEnsembleRegressor\): unsupported operator form: the ensemble has no nodes"),
    ("base", _stump(base_values=[1.0, 2.0]), r"base_values holds 2 values, expected 1"),
]


@pytest.mark.parametrize("name,attrs,pattern", REJECTS, ids=[r[0] for r in REJECTS])
def test_rejections(api, tmp_path, name, attrs, pattern):
    _reject(api, tmp_path, name, _attrs(attrs), pattern)


def test_reject_node_cap(api, tmp_path):
    n = 131072 + 1  # one tree above the per-tree cap: a chain of LT nodes
    ids = list(range(n))
    a = {"nodes_treeids": [0] * n, "nodes_nodeids": ids, "nodes_featureids": [0] * n,
         "nodes_modes": ["BRANCH_LT"] * (n - 1) + ["LEAF"], "nodes_values": [0.0] * n,
         "nodes_truenodeids": [i + 1 for i in range(n - 1)] + [0], "nodes_falsenodeids": [0] * n,
         "target_treeids": [], "target_nodeids": [], "target_ids": [], "target_weights": []}
    # (the false child 0 would be a second parent of the root: give every branch its own leaf instead)
    a["nodes_treeids"] += [0] * (n - 1)
    a["nodes_nodeids"] += [n + i for i in range(n - 1)]
    a["nodes_featureids"] += [0] * (n - 1)
    a["nodes_modes"] += ["LEAF"] * (n - 1)
    a["nodes_values"] += [0.0] * (n - 1)
    a["nodes_truenodeids"] += [0] * (n - 1)
    a["nodes_falsenodeids"] = [n + i for i in range(n - 1)] + [0] + [0] * (n - 1)
    _reject(api, tmp_path, "cap", _attrs(a), rf"tree 0 has {2 * n - 1} nodes, above the cap of 131071")


def test_reject_classifier_forms(api, tmp_path):
    base = {"nodes_treeids": [0, 0, 0], "nodes_nodeids": [0, 1, 2], "nodes_featureids": [1, 0, 0],
            "nodes_modes": ["BRANCH_LEQ", "LEAF", "LEAF"], "nodes_values": [0.5, 0, 0], "nodes_truenodeids": [1, 0, 0],
            "nodes_falsenodeids": [2, 0, 0], "class_treeids": [0, 0], "class_nodeids": [1, 2], "class_ids": [1, 1],
            "class_weights": [0.2, 0.7], "classlabels_int64s": [0, 1]}
    cases = [
        ("strings", {"classlabels_int64s": None, "classlabels_strings": ["a", "b"]}, r"string class labels"),
        ("ambiguous", {"post_transform": "LOGISTIC"}, r"binary single-column form with non-negative weights and post_transform LOGISTIC"),
        ("binbase", {"base_values": [0.1, 0.2]}, r"at most one base_values entry"),
        ("classid", {"class_ids": [0, 2]}, r"class id 2 is not below E = 2"),
    ]
    for name, over, pat in cases:
        a = dict(base)
        for k, v in over.items():
            if v is None:
                a.pop(k)
            else:
                a[k] = v
        attrs = []
        for k, v in a.items():
            attrs += [W.attr_strings(k, v)] if k == "classlabels_strings" else _attrs({k: v})
        _reject(api, tmp_path, "c_" + name, attrs, pat, op="TreeEnsembleClassifier")


def test_reject_input_rank(api, tmp_path):
    _reject(api, tmp_path, "rank", _attrs(_stump()), r"only \[rows, features\] activations", in_dims=["N", 2, 2])


def test_opset5_tree_ensemble_still_unsupported(api, tmp_path):
    nd = W.node("TreeEnsemble", ["X"], ["Y"], [], domain=W.ML_DOMAIN)
    p = W.write(str(tmp_path / "te5.onnx"), W.model("te5", [nd], [], [W.value_info("X", ["N", 4])], [W.value_info("Y", ["N", 1])], ml_opset=5))
    with pytest.raises(api.InferaError, match=r"TreeEnsemble\): unsupported operator"):
        api.load_model("te5", p)


def test_hostile_strings_attribute_is_bounds_checked(api, tmp_path):
    """A `strings` entry whose length runs past the attribute is a decode error, not a read past the buffer."""
    good = W.attr_strings("nodes_modes", ["LEAF"])
    bad = good.replace(b"\x4a\x04LEAF", b"\x4a\x7fLEAF")
    assert bad != good
    nd = W.node("TreeEnsembleRegressor", ["X"], ["Y"], [bad], domain=W.ML_DOMAIN)
    p = W.write(str(tmp_path / "hostile.onnx"), W.model("h", [nd], [], [W.value_info("X", ["N", 4])], [W.value_info("Y", ["N", 1])], ml_opset=1))
    with pytest.raises(api.InferaError, match=r"protobuf decode"):
        api.load_model("hostile", p)
