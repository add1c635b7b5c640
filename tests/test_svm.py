"""ai.onnx.ml SVMRegressor / SVMClassifier at load time (no GPU): the plan a seeded model lowers to, output selection, and every form
that is rejected with its reason."""
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


def _svm_steps(plan):
    steps = plan["plan"]["steps"]
    k = [s for s in steps if s["kind"] == "SvmKernel"]
    assert len(k) == 1, steps
    return k[0], steps


def test_rbf_svr_plan(api, tmp_path):
    spec = W.svm_spec(features=128, n_sv=16384, kind="regressor", kernel="RBF", seed=3)
    plan = _load(api, tmp_path, "svr", W.svm_from_spec(spec))
    k, steps = _svm_steps(plan)
    assert [s["kind"] for s in steps] == ["SvmKernel", "SvmReduce"]
    assert k["kernel"] == "RBF" and k["support_vectors"] == 16384 and k["F"] == 128 and k["classes"] == 1
    assert k["output"] == "value" and k["probabilities"] is False and k["slices"] == 16
    assert plan["plan"]["input_shape"] == [-1, 128] and plan["plan"]["output_shape"] == [-1, 1]
    assert plan["plan"]["flops_per_row"] == 2 * 16384 * (128 + 1)


def test_svc_plan_and_output_selection(api, tmp_path):
    spec = W.svm_spec(features=30, n_sv=4096, classes=3, kernel="RBF", probabilities=True, post="SOFTMAX", labels=[3, 7, 42], seed=4)
    blob = W.svm_from_spec(spec)
    plan = _load(api, tmp_path, "svc", blob)
    k, steps = _svm_steps(plan)
    assert [s["kind"] for s in steps] == ["SvmKernel", "SvmReduce"]  # label only: no Softmax step
    assert k["output"] == "label" and k["classes"] == 3 and k["probabilities"] is True and k["F"] == 30
    assert plan["plan"]["output_shape"] == [-1]
    plan = _load(api, tmp_path, "svc_p", blob, "#probabilities")
    k, steps = _svm_steps(plan)
    assert [s["kind"] for s in steps] == ["SvmKernel", "SvmReduce", "Softmax"]
    assert k["output"] == "probabilities" and plan["plan"]["output_shape"] == [-1, 3]
    # the slices are fixed by the model: each inside one class block
    assert k["slices"] >= 3


@pytest.mark.parametrize("C,prob,cols", [(2, False, 2), (2, True, 2), (4, False, 6), (4, True, 4), (7, False, 21)])
def test_score_shapes(api, tmp_path, C, prob, cols):
    spec = W.svm_spec(features=5, n_sv=40, classes=C, kernel="POLY", probabilities=prob, seed=C)
    plan = _load(api, tmp_path, f"s{C}{int(prob)}", W.svm_from_spec(spec), "#probabilities")
    k, _ = _svm_steps(plan)
    assert k["output"] == ("probabilities" if prob else "decision")
    assert plan["plan"]["output_shape"] == [-1, cols]


def test_one_class_and_scaler_pipeline(api, tmp_path):
    spec = W.svm_spec(features=6, n_sv=50, kind="one_class", kernel="RBF", seed=5)
    plan = _load(api, tmp_path, "oc", W.svm_from_spec(spec, scaler=([0.5] * 6, [2.0] * 6)))
    k, steps = _svm_steps(plan)
    assert k["output"] == "one_class" and steps[0]["kind"] != "SvmKernel"


# ---- rejections ----------------------------------------------------------------------------------------------------------------

def _base(op="SVMClassifier", F=2):
    a = {"kernel_type": "RBF", "kernel_params": [0.5, 0.0, 3.0], "support_vectors": [0.0, 1.0, 1.0, 0.0, 2.0, 2.0],
         "rho": [0.1], "post_transform": "NONE"}
    if op == "SVMClassifier":
        a.update({"coefficients": [1.0, -1.0, 0.5], "vectors_per_class": [1, 2], "classlabels_ints": [0, 1]})
    else:
        a.update({"coefficients": [1.0, -1.0, 0.5], "n_supports": 3})
    return a


def _attrs(a):
    out = []
    for k, v in a.items():
        if isinstance(v, str):
            out.append(W.attr_s(k, v))
        elif isinstance(v, int):
            out.append(W.attr_i(k, v))
        elif k in ("vectors_per_class", "classlabels_ints"):
            out.append(W.attr_ints(k, v))
        elif k == "classlabels_strings":
            out.append(W.attr_strings(k, v))
        else:
            out.append(W.attr_floats(k, v))
    return out


def _reject(api, tmp_path, name, a, pattern, op="SVMClassifier", in_dims=None, F=2):
    outs = ["label", "scores"] if op == "SVMClassifier" else ["Y"]
    nd = W.node(op, ["X"], outs, _attrs(a), domain=W.ML_DOMAIN)
    out_vi = W.value_info(outs[0], ["N"] if op == "SVMClassifier" else ["N", 1], W.INT64 if op == "SVMClassifier" else W.FLOAT)
    blob = W.model(name, [nd], [], [W.value_info("X", in_dims or ["N", F])], [out_vi], ml_opset=1)
    p = W.write(str(tmp_path / f"{name}.onnx"), blob)
    with pytest.raises(api.InferaError, match=pattern):
        api.load_model("bad_" + name, p)


def _over(op="SVMClassifier", drop=(), **kw):
    a = _base(op)
    for k in drop:
        a.pop(k)
    a.update(kw)
    return a


FORM = r"unsupported operator form: "
REJECTS = [
    ("kernel_type", _over(kernel_type="CUBIC"), FORM + r"unknown kernel_type 'CUBIC'"),
    ("no_params", _over(drop=("kernel_params",)), FORM + r"RBF kernel without kernel_params"),
    ("params_len", _over(kernel_params=[0.5, 0.0]), FORM + r"kernel_params holds 2 values, expected 3"),
    ("degree_frac", _over(kernel_type="POLY", kernel_params=[0.5, 0.0, 2.5]), FORM + r"POLY degree 2.5\d* is not an integer from 1 to 16"),
    ("degree_big", _over(kernel_type="POLY", kernel_params=[0.5, 0.0, 17.0]), FORM + r"POLY degree 17.0* is not an integer"),
    ("degree_zero", _over(kernel_type="POLY", kernel_params=[0.5, 0.0, 0.0]), FORM + r"POLY degree 0.0* is not an integer"),
    ("sv_len", _over(support_vectors=[0.0, 1.0, 1.0, 0.0, 2.0]), FORM + r"support_vectors holds 5 values, not a multiple of the input width 2"),
    ("sv_width", _over(support_vectors=[0.0] * 9, vectors_per_class=[1, 1, 1], classlabels_ints=[0, 1, 2], coefficients=[0.0] * 6, rho=[0.0] * 3),
     FORM + r"support_vectors holds 9 values, not a multiple of the input width 2"),
    ("sv_count", _over(support_vectors=[0.0] * 8), FORM + r"support_vectors holds 4 vectors of the input width 2, but vectors_per_class sums to 3"),
    ("no_sv", _over(drop=("support_vectors",), vectors_per_class=[0, 0], coefficients=[]), FORM + r"no support vectors"),
    ("no_vpc", _over(drop=("vectors_per_class",)), FORM + r"no support vectors"),
    ("vpc_len", _over(vectors_per_class=[1, 1, 1]), FORM + r"vectors_per_class holds 3 entries, expected C = 2"),
    ("vpc_neg", _over(vectors_per_class=[-1, 4]), FORM + r"vectors_per_class holds a negative entry \(-1\)"),
    ("vpc_sum", _over(vectors_per_class=[1, 1]), FORM + r"support_vectors holds 3 vectors of the input width 2, but vectors_per_class sums to 2"),
    ("reg_sv_count", _over("SVMRegressor", n_supports=2, coefficients=[1.0, 2.0]), FORM + r"support_vectors holds 3 vectors of the input width 2, but n_supports is 2"),
    ("coef_len", _over(coefficients=[1.0, 2.0]), FORM + r"coefficients holds 2 values, expected \(C - 1\) x n_SV = 3"),
    ("rho_len", _over(rho=[0.1, 0.2]), FORM + r"rho holds 2 values, expected 1"),
    ("prob_a_only", _over(prob_a=[-1.0]), FORM + r"only prob_a is given"),
    ("prob_b_only", _over(prob_b=[0.1]), FORM + r"only prob_b is given"),
    ("prob_len", _over(prob_a=[-1.0, -1.0], prob_b=[0.1, 0.1]), FORM + r"prob_a holds 2 values, expected 1"),
    ("prob_b_len", _over(prob_a=[-1.0], prob_b=[0.1, 0.1]), FORM + r"prob_b holds 2 values, expected 1"),
    ("strings", _over(drop=("classlabels_ints",), classlabels_strings=["a", "b"]), FORM + r"string class labels"),
    ("one_class", _over(classlabels_ints=[0], vectors_per_class=[3], coefficients=[]), FORM + r"needs at least two classlabels_ints"),
    ("softmax_zero", _over(post_transform="SOFTMAX_ZERO"), FORM + r"post_transform SOFTMAX_ZERO"),
    ("probit", _over(post_transform="PROBIT"), FORM + r"post_transform PROBIT"),
    ("reg_coef", _over("SVMRegressor", coefficients=[1.0, 2.0]), FORM + r"coefficients holds 2 values, expected n_SV = 3"),
    ("reg_rho", _over("SVMRegressor", rho=[]), FORM + r"rho holds 0 values, expected 1"),
    ("reg_no_sv", _over("SVMRegressor", drop=("support_vectors",), n_supports=0, coefficients=[]), FORM + r"no support vectors"),
]


@pytest.mark.parametrize("name,attrs,pattern", REJECTS, ids=[r[0] for r in REJECTS])
def test_rejections(api, tmp_path, name, attrs, pattern):
    op = "SVMRegressor" if name.startswith("reg_") else "SVMClassifier"
    _reject(api, tmp_path, name, attrs, pattern, op=op)


def test_reject_input_rank(api, tmp_path):
    _reject(api, tmp_path, "rank", _base(), r"only \[rows, features\] activations", in_dims=["N", 1, 2])


def test_reject_caps(api, tmp_path):
    # input width above 1024
    a = _over(support_vectors=[0.0] * (3 * 1025))
    _reject(api, tmp_path, "cap_f", a, FORM + r"input width 1025 is above the cap of 1024", F=1025)
    # more than 64 classes
    C = 65
    a = _over(classlabels_ints=list(range(C)), vectors_per_class=[1] * C, support_vectors=[0.0] * (2 * C),
              coefficients=[0.0] * ((C - 1) * C), rho=[0.0] * (C * (C - 1) // 2))
    _reject(api, tmp_path, "cap_c", a, FORM + r"C = 65 classes, above the cap of 64")
    # probabilities above 16 classes
    C = 17
    P = C * (C - 1) // 2
    a = _over(classlabels_ints=list(range(C)), vectors_per_class=[1] * C, support_vectors=[0.0] * (2 * C),
              coefficients=[0.0] * ((C - 1) * C), rho=[0.0] * P, prob_a=[-1.0] * P, prob_b=[0.0] * P)
    _reject(api, tmp_path, "cap_p", a, FORM + r"probabilities for C = 17 classes, above the cap of 16")
    # more than 262144 support vectors
    n = 262145
    a = _over("SVMRegressor", kernel_type="LINEAR", drop=("kernel_params",), n_supports=n, coefficients=np.zeros(n, np.float32),
              support_vectors=np.zeros(n, np.float32))
    _reject(api, tmp_path, "cap_sv", a, FORM + r"n_SV = 262145 support vectors, above the cap of 262144", op="SVMRegressor", F=1)


def test_caps_accepted(api, tmp_path):
    """The documented minimum caps load: F = 1024, C = 64 without and C = 16 with probabilities."""
    spec = W.svm_spec(features=1024, n_sv=40, kind="regressor", kernel="RBF", seed=1)
    assert _svm_steps(_load(api, tmp_path, "f1024", W.svm_from_spec(spec)))[0]["F"] == 1024
    spec = W.svm_spec(features=3, n_sv=128, classes=64, kernel="LINEAR", seed=2)
    assert _svm_steps(_load(api, tmp_path, "c64", W.svm_from_spec(spec), "#probabilities"))[0]["classes"] == 64
    spec = W.svm_spec(features=3, n_sv=64, classes=16, kernel="SIGMOID", probabilities=True, seed=3)
    assert _svm_steps(_load(api, tmp_path, "c16", W.svm_from_spec(spec), "#probabilities"))[0]["probabilities"] is True


def test_linear_kernel_needs_no_params(api, tmp_path):
    a = _over(kernel_type="LINEAR", drop=("kernel_params",))
    nd = W.node("SVMClassifier", ["X"], ["label", "scores"], _attrs(a), domain=W.ML_DOMAIN)
    blob = W.model("lin", [nd], [], [W.value_info("X", ["N", 2])], [W.value_info("label", ["N"], W.INT64)], ml_opset=1)
    k, _ = _svm_steps(_load(api, tmp_path, "lin", blob))
    assert k["kernel"] == "LINEAR" and k["support_vectors"] == 3
