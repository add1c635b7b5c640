"""SVMRegressor / SVMClassifier on the GPU (hip/svm.hip) against the float64 numpy restatement of the contract in tests/svm_ref.py
(INTEGRATION.md section 2.6), and bit-reproducibility across every call path."""
from __future__ import annotations

import numpy as np
import pytest

from infera_amd import onnx_writer as W
from infera_amd import synth
from tests.svm_ref import check, np_svm, tol_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api(built):
    from infera_amd import capi

    assert capi.device_count() >= 1, capi.get_devices()
    return capi


def _table(rows, F, seed=23, nan_frac=0.0, offset=0.0):
    x = synth.table(seed, 0, rows, F) + np.float32(offset)
    if nan_frac:
        rng = np.random.default_rng(seed)
        x[rng.random(x.shape[0]) < nan_frac, int(rng.integers(F))] = np.nan
    return x.astype(np.float32)


def _run(api, tmp_path, spec, x, select="", scaler=None, name="svm"):
    p = W.write(str(tmp_path / f"{name}.onnx"), W.svm_from_spec(spec, scaler=scaler, output="label"))
    api.load_model(name, p + select)
    try:
        return api.predict(name, x)
    finally:
        api.unload_model(name)


def _sv_like(spec, x):
    """support vectors drawn from the table (as a fitted SVM's are), so RBF values are not all ~0"""
    rng = np.random.default_rng(spec["n_sv"])
    x = x[np.isfinite(x).all(1)]
    spec["support_vectors"] = x[rng.integers(0, x.shape[0], spec["n_sv"])].astype(np.float32)
    return spec


# ---- every kernel x every form -------------------------------------------------------------------------------------------------

FORMS = [("regressor", 1, False), ("one_class", 1, False), ("classifier", 2, False), ("classifier", 2, True), ("classifier", 3, False),
         ("classifier", 3, True), ("classifier", 7, False), ("classifier", 7, True)]


@pytest.mark.parametrize("kernel", W.SVM_KERNELS)
@pytest.mark.parametrize("form", FORMS, ids=lambda f: f"{f[0]}{f[1] if f[0] == 'classifier' else ''}{'_prob' if f[2] else ''}")
def test_kernel_and_form(api, tmp_path, kernel, form):
    kind, C, prob = form
    F = 13
    x = _table(2049, F, seed=5 + C, nan_frac=0.01)
    spec = _sv_like(W.svm_spec(features=F, n_sv=80, kind=kind, classes=C, kernel=kernel, probabilities=prob, degree=3,
                               gamma=0.05 if kernel != "RBF" else None, seed=11 + C), x)
    ref = np_svm(spec, x)
    if kind == "classifier":
        check(spec, ref, _run(api, tmp_path, spec, x), "label")
        check(spec, ref, _run(api, tmp_path, spec, x, "#probabilities"), "scores")
    else:
        check(spec, ref, _run(api, tmp_path, spec, x), "scores")


@pytest.mark.parametrize("post", ["LOGISTIC", "SOFTMAX"])
@pytest.mark.parametrize("prob", [False, True])
def test_post_transform(api, tmp_path, post, prob):
    F, C = 10, 4
    x = _table(3000, F, seed=7)
    spec = _sv_like(W.svm_spec(features=F, n_sv=200, classes=C, kernel="RBF", probabilities=prob, post=post, seed=8), x)
    ref = np_svm(spec, x)
    got = _run(api, tmp_path, spec, x, "#probabilities").astype(np.float64)
    s = ref["scores"]
    want = 1 / (1 + np.exp(-s)) if post == "LOGISTIC" else np.exp(s - s.max(1, keepdims=True)) / np.exp(s - s.max(1, keepdims=True)).sum(1, keepdims=True)
    tol = tol_of(ref).max(1, keepdims=True) * (10 if prob else 2) + 1e-6
    assert np.all(np.abs(got - want) <= tol), np.abs(got - want).max()
    check(spec, ref, _run(api, tmp_path, spec, x), "label")  # the label is taken before post_transform


# ---- awkward sizes ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("F", [1, 13, 30, 129])
@pytest.mark.parametrize("n_sv", [1, 33, 4097])
def test_sizes_regressor(api, tmp_path, F, n_sv):
    x = _table(1000, F, seed=F + n_sv)
    spec = _sv_like(W.svm_spec(features=F, n_sv=n_sv, kind="regressor", kernel="RBF", seed=F), x)
    check(spec, np_svm(spec, x), _run(api, tmp_path, spec, x), "scores")


@pytest.mark.parametrize("per_class", [[1, 40, 2], [33, 1, 64, 0, 5], [100, 1]], ids=["1_40_2", "33_1_64_0_5", "100_1"])
def test_uneven_class_blocks(api, tmp_path, per_class):
    F = 9
    x = _table(2000, F, seed=len(per_class))
    spec = _sv_like(W.svm_spec(features=F, n_sv=sum(per_class), classes=len(per_class), per_class=per_class, kernel="RBF", seed=3), x)
    ref = np_svm(spec, x)
    check(spec, ref, _run(api, tmp_path, spec, x, "#probabilities"), "scores")
    check(spec, ref, _run(api, tmp_path, spec, x), "label")


@pytest.mark.parametrize("rows", [1, 63, 64, 65, 2049, 100000])
def test_row_counts(api, tmp_path, rows):
    F = 30
    x = _table(rows, F, seed=rows % 97)
    spec = _sv_like(W.svm_spec(features=F, n_sv=500, classes=3, kernel="RBF", probabilities=True, seed=9), _table(4096, F, seed=3))
    ref = np_svm(spec, x)
    check(spec, ref, _run(api, tmp_path, spec, x, "#probabilities"), "scores")


def test_many_classes_mfma_stage2(api, tmp_path):
    """C - 1 above 8 coefficient rows: the second MFMA (one and two 32-row tiles)"""
    for C in (12, 40):
        F = 16
        x = _table(1500, F, seed=C)
        spec = _sv_like(W.svm_spec(features=F, n_sv=20 * C, classes=C, kernel="RBF", seed=C), x)
        ref = np_svm(spec, x)
        dec = _run(api, tmp_path, spec, x, "#probabilities")
        check(spec, ref, dec, "scores")
        # with C (C - 1) / 2 pairs some decision is near 0 on many rows: the label must follow the votes of the served decisions
        votes = np.zeros((x.shape[0], C), dtype=np.int64)
        p = 0
        for i in range(C):
            for j in range(i + 1, C):
                votes[np.arange(x.shape[0]), np.where(dec[:, p] > 0, i, j)] += 1
                p += 1
        label = _run(api, tmp_path, spec, x).reshape(-1)
        assert np.array_equal(label, np.argmax(votes, 1).astype(np.float32))


def test_offset_features_rbf(api, tmp_path):
    """1000 + N(0, 1) features: |x|^2 + |s|^2 - 2 x.s in f32 loses every digit without the load-time center"""
    F = 20
    x = _table(3000, F, seed=13, offset=1000.0)
    spec = W.svm_spec(features=F, n_sv=400, kind="regressor", kernel="RBF", offset=1000.0, gamma=0.05, seed=14)
    ref = np_svm(spec, x)
    assert np.median(np.abs(ref["d"])) > 1e-2  # the kernel values are not all ~0
    check(spec, ref, _run(api, tmp_path, spec, x), "scores")


def test_nan_rows(api, tmp_path):
    F, C = 8, 4
    x = _table(500, F, seed=17)
    x[::7, 3] = np.nan
    for prob in (False, True):
        spec = _sv_like(W.svm_spec(features=F, n_sv=120, classes=C, kernel="RBF", probabilities=prob, labels=[5, 6, 7, 8], seed=18), x[1::7])
        label = _run(api, tmp_path, spec, x).reshape(-1)
        scores = _run(api, tmp_path, spec, x, "#probabilities")
        assert np.isnan(scores[::7]).all() and not np.isnan(scores[1::7]).any()
        assert (label[::7] == 8).all()  # every comparison false: class C - 1
    spec = _sv_like(W.svm_spec(features=F, n_sv=60, kind="one_class", kernel="RBF", seed=19), x[1::7])
    assert (_run(api, tmp_path, spec, x)[::7, 0] == -1).all()


def test_scaler_pipeline(api, tmp_path):
    F = 12
    x = _table(3000, F, seed=21) * np.float32(3) + np.float32(5)
    off = np.linspace(4.0, 6.0, F).astype(np.float32)
    sc = np.linspace(0.2, 0.5, F).astype(np.float32)
    shift = (-off.astype(np.float64) * sc).astype(np.float32)  # the Scaler runs as x * scale + f32(-offset * scale)
    xs = (x.astype(np.float64) * sc + shift).astype(np.float32)
    spec = _sv_like(W.svm_spec(features=F, n_sv=300, classes=3, kernel="RBF", probabilities=True, seed=22), xs)
    ref = np_svm(spec, xs)
    check(spec, ref, _run(api, tmp_path, spec, x, scaler=(off, sc)), "label")
    check(spec, ref, _run(api, tmp_path, spec, x, "#probabilities", scaler=(off, sc)), "scores")


# ---- reproducibility -----------------------------------------------------------------------------------------------------------

def test_bits_independent_of_call_path(api, tmp_path):
    from infera_amd import sqlharness

    F, rows = 30, 100_000
    x = _table(rows, F, seed=29)
    spec = _sv_like(W.svm_spec(features=F, n_sv=1000, classes=3, kernel="RBF", probabilities=True, seed=30), x[:5000])
    p = W.write(str(tmp_path / "rep.onnx"), W.svm_from_spec(spec, output="probabilities"))
    api.load_model("rep", p)
    try:
        ref = api.predict("rep", x)
        for step in (1, 7, 2048, 2049):
            n = rows if step > 1 else 3000
            parts = [api.predict("rep", x[i:i + step]) for i in range(0, n, step)]
            assert np.array_equal(np.concatenate(parts), ref[:n]), step
        assert np.array_equal(api.predict_from_blob("rep", x[:20000].tobytes()), ref[:20000])
        cols = [np.ascontiguousarray(x[:, j]) for j in range(F)]
        assert np.array_equal(api.predict_columns("rep", cols), ref)
        api.register_host_memory(x)
        try:
            assert np.array_equal(api.predict("rep", x), ref)
            assert np.array_equal(api.predict_columns("rep", cols), ref)
        finally:
            api.unregister_host_memory(x)
        for d in range(api.device_count()):
            dev = api.device_ordinal(d)
            d_in, d_out = api.DeviceBuffer(dev, x.nbytes), api.DeviceBuffer(dev, rows * 3 * 4)
            d_in.upload(x)
            api.predict_device("rep", d_in, rows, F, d_out)
            assert np.array_equal(d_out.download((rows, 3)), ref), f"device slot {d}"
    finally:
        api.unload_model("rep")
    pl = W.write(str(tmp_path / "rep_label.onnx"), W.svm_from_spec(spec, output="label"))
    api.load_model("rep_l", pl)
    try:
        lab = api.predict("rep_l", x)
    finally:
        api.unload_model("rep_l")
    sqlharness.sql("infera_load_model", "rep_sql", pl)
    try:
        got = sqlharness.sql("infera_predict", "rep_sql", *[np.ascontiguousarray(x[4096:6144, j]) for j in range(F)])
    finally:
        sqlharness.sql("infera_unload_model", "rep_sql")
    assert np.array_equal(np.asarray(got, dtype=np.float32), lab[4096:6144].reshape(-1))
    r = np_svm(spec, x[:3000])
    check(spec, r, ref[:3000], "scores")
    check(spec, r, lab[:3000], "label")


# ---- optional: scikit-learn estimators written through the builder --------------------------------------------------------------

def _sk_spec(est, F, kind):
    coef = np.asarray(est._dual_coef_, dtype=np.float64)
    spec = {"kind": kind, "features": F, "kernel": est.kernel.upper(), "post": "NONE", "n_sv": int(est.support_vectors_.shape[0]),
            "support_vectors": np.asarray(est.support_vectors_, dtype=np.float32),
            "coefficients": coef.astype(np.float32), "rho": np.asarray(est._intercept_, dtype=np.float32).ravel(),
            "kernel_params": np.asarray([est._gamma, est.coef0, est.degree], dtype=np.float32), "prob_a": None, "prob_b": None}
    if kind == "classifier":
        spec.update(classes=len(est.classes_), labels=[int(c) for c in est.classes_], vectors_per_class=[int(v) for v in est.n_support_])
        if getattr(est, "probability", False):
            spec.update(prob_a=np.asarray(est.probA_, np.float32), prob_b=np.asarray(est.probB_, np.float32))
    return spec


def test_sklearn_cross_check(api, tmp_path):
    svm = pytest.importorskip("sklearn.svm")
    F = 6
    x = _table(400, F, seed=41)
    y3 = np.digitize(x[:, 0] + 0.5 * x[:, 1] * x[:, 2], [-0.5, 0.5])
    for est, kind in [(svm.SVC(kernel="rbf", probability=True, random_state=0, decision_function_shape="ovo").fit(x, y3), "classifier"),
                      (svm.SVC(kernel="poly", degree=2).fit(x, y3 > 0), "classifier"),
                      (svm.SVR(kernel="rbf").fit(x, x[:, 0] * x[:, 1]), "regressor"),
                      (svm.OneClassSVM(kernel="rbf", nu=0.2).fit(x), "regressor")]:
        spec = _sk_spec(est, F, kind)
        if kind == "classifier" and len(est.classes_) == 2:
            spec["labels"] = [0, 1]
        ref = np_svm(spec, x)
        name = type(est).__name__
        if kind == "classifier":
            lab = _run(api, tmp_path, spec, x, name=name).reshape(-1)
            near = (np.abs(ref["d"]) <= tol_of(ref)).any(1)
            print(f"{name}({est.kernel}): {int(near.sum())} rows excluded")
            want = est.predict(x).astype(np.float32)
            assert np.array_equal(lab[~near], want[~near])
            dec = est.decision_function(x)
            if spec["classes"] > 2:
                got = _run(api, tmp_path, dict(spec, prob_a=None, prob_b=None), x, "#probabilities", name=name + "_d")
                assert np.all(np.abs(got - dec) <= tol_of(ref))
            else:
                got = _run(api, tmp_path, dict(spec, prob_a=None, prob_b=None), x, "#probabilities", name=name + "_d")[:, 1]
                assert np.all(np.abs(got - dec) <= tol_of(ref)[:, 0])  # column 1 = -d_01 = sklearn binary decision_function
            if spec.get("prob_a") is not None:
                proba = _run(api, tmp_path, spec, x, "#probabilities", name=name + "_p")
                assert np.abs(proba - est.predict_proba(x)).max() < 1e-2
        else:
            got = _run(api, tmp_path, spec, x, name=name)[:, 0]
            want = est.predict(x) if isinstance(est, svm.SVR) else est.decision_function(x)
            assert np.all(np.abs(got - want.ravel()) <= tol_of(ref)[:, 0])
