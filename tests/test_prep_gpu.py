"""ai.onnx.ml preprocessing regions on the GPU (hip/prep.hip) against a numpy f32 restatement of the contract (INTEGRATION.md section 2.6
"Preprocessing"), bit for bit; bit-reproducibility across every call path and row count; the zeros = 0 failure; ZipMap outputs; and a
scikit-learn cross-check of ColumnTransformer pipelines written by onnx_writer.sklearn_column_transformer."""
from __future__ import annotations

import numpy as np
import pytest

from infera_amd import onnx_writer as W

pytestmark = pytest.mark.gpu

f32 = np.float32


@pytest.fixture(scope="module")
def api(built):
    from infera_amd import capi

    assert capi.device_count() >= 1, capi.get_devices()
    return capi


# ---- the restatement: one rounded f32 operation per step -----------------------------------------------------------------------

def np_lookup(k, keys, vals, dflt, nan_val=None):
    keys = np.asarray(keys, f32)
    out = np.full(k.shape, f32(dflt), f32)
    for key, v in zip(keys, np.asarray(vals, f32)):
        out[k == key] = v
    if nan_val is not None:
        out[np.isnan(k)] = f32(nan_val)
    return out


def np_prep(spec, x):
    g = spec["groups"]
    parts = []
    if g["numeric"]:
        v = x[:, g["numeric"]]
        v = np.where(np.isnan(v), np.asarray(spec["imputed"], f32), v).astype(f32)
        v = (v - np.asarray(spec["offset"], f32)).astype(f32)
        parts.append((v * np.asarray(spec["scale"], f32)).astype(f32))
    for col, cats in zip(g["categorical"], spec["cats"]):
        t = np.trunc(x[:, col])
        parts.append((t[:, None] == np.asarray(cats, f32)[None, :]).astype(f32))
    for col, t in zip(g["ordinal"], spec["ordinal"]):
        k = x[:, col] if t["floats"] else np.trunc(x[:, col])
        parts.append(np_lookup(k, t["keys"], t["values"], t["default"])[:, None])
    for col, thr in zip(g["binarized"], spec["thresholds"]):
        parts.append((x[:, col] > f32(thr)).astype(f32)[:, None])
    return np.concatenate(parts, axis=1)


def hostile_table(spec, rows, seed=3):
    """Rows with NaN, +-0, +-inf, non-integral and negative categories, unknown categories and LabelEncoder misses."""
    rng = np.random.default_rng(seed)
    x = rng.normal(0, 1, (rows, spec["features"])).astype(f32)
    g = spec["groups"]
    special = np.asarray([np.nan, 0.0, -0.0, np.inf, -np.inf], f32)
    for c in g["numeric"] + g["binarized"]:
        m = rng.random(rows) < 0.15
        x[m, c] = rng.choice(special, int(m.sum()))
    for cats, c in zip(spec["cats"], g["categorical"]):
        pool = np.concatenate([np.asarray(cats, f32), np.asarray(cats, f32) + f32(0.4), np.asarray(cats, f32) - f32(0.6),
                               np.asarray([99, -99, 1e9, -1e9], f32), special])
        x[:, c] = rng.choice(pool, rows)
    for t, c in zip(spec["ordinal"], g["ordinal"]):
        pool = np.concatenate([np.asarray(t["keys"], f32), np.asarray(t["keys"], f32) + f32(0.5), np.asarray([77, -77], f32), special])
        x[:, c] = rng.choice(pool, rows)
    return x


def bits_equal(a, b):
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _load(api, tmp_path, name, blob, select=""):
    p = W.write(str(tmp_path / f"{name}.onnx"), blob)
    api.load_model(name, p + select)
    return p


SPEC = W.prep_spec(binarized=2)  # the reference shape plus two Binarizer columns


# ---- each operator and the reference shape, bit for bit ----------------------------------------------------------------------

@pytest.mark.parametrize("layout", [dict(), dict(after_onehot="Flatten", concat_axis=-1), dict(after_onehot="Squeeze", cast=False)],
                         ids=["reshape", "flatten", "squeeze"])
def test_reference_shape_bits(api, tmp_path, layout):
    x = hostile_table(SPEC, 5003)
    _load(api, tmp_path, "ref", W.prep_from_spec(SPEC, **layout))
    try:
        got = api.predict("ref", x)
    finally:
        api.unload_model("ref")
    want = np_prep(SPEC, x)
    assert got.shape == want.shape == (5003, W.prep_width(SPEC))
    assert bits_equal(got, want)


def _single(op, attrs, width, out_width=None, x_type=W.FLOAT):
    nodes = [W.node(op, ["X"], ["Y"], attrs, name="n", domain=W.ML_DOMAIN)]
    return W.model("one", nodes, [], [W.value_info("X", ["N", width], x_type)], [W.value_info("Y", ["N", out_width or width])], ml_opset=3)


def test_imputer_forms(api, tmp_path):
    x = np.asarray([[0.0, -0.0, np.nan], [2.0, 3.5, -0.0], [np.inf, 2.0, 2.0]], f32)
    for name, attrs, want in [
        # replaced_value_float defaults to 0 (the specification): 0 and -0 are imputed, NaN is kept
        ("default", [W.attr_floats("imputed_value_floats", [7.0])], np.where(x == 0, f32(7), x)),
        ("nan", [W.attr_floats("imputed_value_floats", [7.0]), W.attr_f("replaced_value_float", float("nan"))],
         np.where(np.isnan(x), f32(7), x)),
        ("zero", [W.attr_floats("imputed_value_floats", [1.0, 2.0, 3.0]), W.attr_f("replaced_value_float", 0.0)],
         np.where(x == 0, np.asarray([1, 2, 3], f32), x)),
        ("int", [W.attr_ints("imputed_value_int64s", [-5]), W.attr_i("replaced_value_int64", 2)], np.where(x == 2, f32(-5), x)),
    ]:
        _load(api, tmp_path, "imp_" + name, _single("Imputer", attrs, 3))
        try:
            assert bits_equal(api.predict("imp_" + name, x), want.astype(f32)), name
        finally:
            api.unload_model("imp_" + name)


def test_binarizer_and_scaler(api, tmp_path):
    x = np.asarray([[np.nan, 0.5, -0.0, 0.3, np.inf, -np.inf]], f32).repeat(3, 0)
    _load(api, tmp_path, "bin", _single("Binarizer", [W.attr_f("threshold", 0.3)], 6))
    try:
        assert bits_equal(api.predict("bin", x), (x > f32(0.3)).astype(f32))
    finally:
        api.unload_model("bin")
    # a Scaler inside a region: (x - offset) * scale as two roundings (a Scaler in a graph without a region lowers as before)
    rng = np.random.default_rng(5)
    x = rng.normal(0, 3, (1000, 3)).astype(f32)
    off, sc = rng.normal(0, 1, 3).astype(f32), rng.uniform(0.1, 3, 3).astype(f32)
    nodes = [W.node("Scaler", ["X"], ["S"], [W.attr_floats("offset", off), W.attr_floats("scale", sc)], domain=W.ML_DOMAIN),
             W.node("LabelEncoder", ["S"], ["Y"], [W.attr_floats("keys_floats", [1e30]), W.attr_floats("values_floats", [0.0]),
                                                  W.attr_f("default_float", 5.0)], domain=W.ML_DOMAIN),
             W.node("Concat", ["S", "Y"], ["Z"], [W.attr_i("axis", 1)])]
    _load(api, tmp_path, "sc", W.model("sc", nodes, [], [W.value_info("X", ["N", 3])], [W.value_info("Z", ["N", 6])], ml_opset=3))
    try:
        got = api.predict("sc", x)
    finally:
        api.unload_model("sc")
    want = ((x - off).astype(f32) * sc).astype(f32)
    assert bits_equal(got[:, :3], want) and np.all(got[:, 3:] == 5)


def test_label_encoder_forms(api, tmp_path):
    x = np.asarray([[0.0, -0.0, np.nan, 1.5, -2.7, 3.0, 7.0, np.inf, -1.0]], f32).T.copy()
    # float keys: f32 equality, -0 == 0, a NaN key matches NaN
    attrs = [W.attr_floats("keys_floats", [-0.0, 1.5, float("nan"), 3.0]), W.attr_floats("values_floats", [10, 11, 12, 13]),
             W.attr_f("default_float", -4.0)]
    _load(api, tmp_path, "lef", _single("LabelEncoder", attrs, 1))
    try:
        assert bits_equal(api.predict("lef", x), np_lookup(x[:, 0], [0.0, 1.5, 3.0], [10, 11, 13], -4.0, nan_val=12)[:, None])
    finally:
        api.unload_model("lef")
    # int64 keys match trunc(x); int64 values are served as f32; NaN misses
    attrs = [W.attr_ints("keys_int64s", [0, -2, 3, 7]), W.attr_ints("values_int64s", [100, -200, 300, 700]), W.attr_i("default_int64", -9)]
    _load(api, tmp_path, "lei", _single("LabelEncoder", attrs, 1))
    try:
        assert bits_equal(api.predict("lei", x), np_lookup(np.trunc(x[:, 0]), [0, -2, 3, 7], [100, -200, 300, 700], -9)[:, None])
    finally:
        api.unload_model("lei")
    # opset-4 tensors
    attrs = [W.attr_tensor("keys_tensor", W.tensor("", np.asarray([1, 3], np.int64))),
             W.attr_tensor("values_tensor", W.tensor("", np.asarray([0.25, 0.5], f32))),
             W.attr_tensor("default_tensor", W.tensor("", np.asarray([2.0], f32)))]
    _load(api, tmp_path, "let", _single("LabelEncoder", attrs, 1))
    try:
        assert bits_equal(api.predict("let", x), np_lookup(np.trunc(x[:, 0]), [1, 3], [0.25, 0.5], 2.0)[:, None])
    finally:
        api.unload_model("let")


def test_integer_inputs_and_afe(api, tmp_path):
    rng = np.random.default_rng(8)
    xi = np.trunc(rng.normal(0, 3, (2049, 3))).astype(f32) + rng.choice(np.asarray([0, 0.5, -0.5], f32), (2049, 3))
    xi[::17, 1] = np.nan
    xf = rng.normal(0, 1, (2049, 2)).astype(f32)
    inits = [W.tensor("ix", np.asarray([2, 0, 2], np.int64))]
    nodes = [W.node("ArrayFeatureExtractor", ["C", "ix"], ["Cp"], domain=W.ML_DOMAIN),
             W.node("Concat", ["Xf", "Cp"], ["Y"], [W.attr_i("axis", 1)])]
    blob = W.model("ii", nodes, inits, [W.value_info("Xf", ["N", 2]), W.value_info("C", ["N", 3], W.INT64)], [W.value_info("Y", ["N", 5])],
                   ml_opset=3)
    _load(api, tmp_path, "ii", blob)
    try:
        got = api.predict("ii", np.concatenate([xf, xi], axis=1))
    finally:
        api.unload_model("ii")
    assert bits_equal(got, np.concatenate([xf, np.trunc(xi[:, [2, 0, 2]])], axis=1))


# ---- reproducibility ---------------------------------------------------------------------------------------------------------

def test_bits_independent_of_call_path(api, tmp_path):
    from infera_amd import sqlharness

    rows = 100_000
    x = hostile_table(SPEC, rows, seed=9)
    F = SPEC["features"]
    p = _load(api, tmp_path, "rep", W.prep_from_spec(SPEC))
    try:
        ref = api.predict("rep", x)
        assert bits_equal(ref, np_prep(SPEC, x))
        for n in (1, 2047, 2048, 2049):
            assert bits_equal(api.predict("rep", x[:n]), ref[:n]), n
            assert bits_equal(api.predict("rep", x[rows - n:]), ref[rows - n:]), n
        parts = [api.predict("rep", x[i:i + 2049]) for i in range(0, 10 * 2049, 2049)]
        assert bits_equal(np.concatenate(parts), ref[:10 * 2049])
        assert bits_equal(api.predict_from_blob("rep", x[:2049].tobytes()), ref[:2049])
        cols = [np.ascontiguousarray(x[:, j]) for j in range(F)]
        assert bits_equal(api.predict_columns("rep", cols), ref)
        api.register_host_memory(x)
        try:
            assert bits_equal(api.predict("rep", x), ref)
            assert bits_equal(api.predict_columns("rep", cols), ref)
        finally:
            api.unregister_host_memory(x)
        for d in range(api.device_count()):
            dev = api.device_ordinal(d)
            for n in (2049, rows):
                d_in = api.DeviceBuffer(dev, n * F * 4)
                d_out = api.DeviceBuffer(dev, n * ref.shape[1] * 4)
                d_in.upload(np.ascontiguousarray(x[:n]))
                api.predict_device("rep", d_in, n, F, d_out)
                assert bits_equal(d_out.download((n, ref.shape[1])), ref[:n]), (d, n)
    finally:
        api.unload_model("rep")
    # the SQL scalar function serves one value per row: the same Prep step in front of a tree regressor, through SQL and the C ABI
    tree = W.tree_ensemble_spec(features=W.prep_width(SPEC), trees=10, depth=5, seed=16)
    p = _load(api, tmp_path, "rep_tree", W.prep_from_spec(SPEC, head=W.tree_head(tree)))
    try:
        want = api.predict("rep_tree", x[4096:6144])
    finally:
        api.unload_model("rep_tree")
    sqlharness.sql("infera_load_model", "rep_sql", p)
    try:
        got = sqlharness.sql("infera_predict", "rep_sql", *[np.ascontiguousarray(x[4096:6144, j]) for j in range(F)])
    finally:
        sqlharness.sql("infera_unload_model", "rep_sql")
    assert bits_equal(np.asarray(got, dtype=f32), want[:, 0])


# ---- zeros = 0 ---------------------------------------------------------------------------------------------------------------

def test_strict_onehot_fails_then_recovers(api, tmp_path):
    spec = W.prep_spec(strict=True, seed=12)
    x = hostile_table(spec, 3000, seed=13)
    good = x.copy()
    for cats, c in zip(spec["cats"], spec["groups"]["categorical"]):
        good[:, c] = np.asarray(cats, f32)[np.arange(3000) % len(cats)]
    _load(api, tmp_path, "strict", W.prep_from_spec(spec))
    try:
        want = np_prep(spec, good)
        assert bits_equal(api.predict("strict", good), want)
        with pytest.raises(api.InferaError, match=r"^ONNX error: node 'cat\d_onehot' \(OneHotEncoder\): a value is not in cats_int64s \(zeros = 0\)$"):
            api.predict("strict", x)
        assert bits_equal(api.predict("strict", good), want)  # the next call works
        bad1 = good.copy()
        bad1[1234, spec["groups"]["categorical"][3]] = np.nan  # a NaN is in no category
        with pytest.raises(api.InferaError, match=r"node 'cat3_onehot'"):
            api.predict("strict", bad1)
        cols = [np.ascontiguousarray(good[:, j]) for j in range(spec["features"])]
        assert bits_equal(api.predict_columns("strict", cols), want)
    finally:
        api.unload_model("strict")


# ---- ZipMap ------------------------------------------------------------------------------------------------------------------

def test_zipmap_equals_probabilities(api, tmp_path):
    tree = W.tree_ensemble_spec(features=W.prep_width(SPEC), trees=20, depth=5, kind="classifier", post="SOFTMAX", seed=14)
    x = hostile_table(SPEC, 4000, seed=15)
    _load(api, tmp_path, "zm", W.prep_from_spec(SPEC, head=W.tree_head(tree), zipmap=True), "#output_probability")
    _load(api, tmp_path, "pr", W.prep_from_spec(SPEC, head=W.tree_head(tree)), "#probabilities")  # the same graph without the ZipMap
    try:
        a, b = api.predict("zm", x), api.predict("pr", x)
        assert a.shape == (4000, 3) and bits_equal(a, b)
    finally:
        api.unload_model("zm")
        api.unload_model("pr")


# ---- scikit-learn cross-check ------------------------------------------------------------------------------------------------

def _sk_data(rows, seed=21):
    rng = np.random.default_rng(seed)
    num = rng.normal(0, 2, (rows, 4))
    num[rng.random(num.shape) < 0.1] = np.nan
    cat = rng.integers(-3, 6, (rows, 3)).astype(np.float64)
    ordc = rng.choice([2, 5, 11, 17], (rows, 1)).astype(np.float64)
    x = np.concatenate([num[:, :2], cat[:, :1], num[:, 2:], cat[:, 1:], ordc], axis=1)  # columns interleaved
    y = (np.nan_to_num(num[:, 0]) + (cat[:, 0] > 1) - 0.3 * ordc[:, 0] / 5 + np.nan_to_num(num[:, 2]) * 0.5)
    return x.astype(f32), y


def _column_transformer(x):
    compose = pytest.importorskip("sklearn.compose")
    from sklearn.impute import SimpleImputer
    from sklearn.pipeline import Pipeline
    from sklearn.preprocessing import OneHotEncoder, OrdinalEncoder, StandardScaler

    ct = compose.ColumnTransformer([
        ("num", Pipeline([("imp", SimpleImputer(strategy="mean")), ("sc", StandardScaler())]), [0, 1, 3, 4]),
        ("cat", OneHotEncoder(handle_unknown="ignore"), [2, 5, 6]),
        ("ord", OrdinalEncoder(), [7]),
    ])
    return ct.fit(x.astype(np.float64))


def _dense(a):
    return a.toarray() if hasattr(a, "toarray") else np.asarray(a)


def test_sklearn_column_transformer_transform(api, tmp_path):
    x, _ = _sk_data(3000)
    ct = _column_transformer(x)
    want = _dense(ct.transform(x.astype(np.float64)))
    xt = x.copy()
    xt[::50, 2] = 40  # unknown categories: all zeros (handle_unknown='ignore')
    want_t = _dense(ct.transform(xt.astype(np.float64)))
    _load(api, tmp_path, "ct", W.sklearn_column_transformer(ct))
    try:
        got = api.predict("ct", x)
        got_t = api.predict("ct", xt)
    finally:
        api.unload_model("ct")
    assert got.shape == want.shape
    # f32 against StandardScaler's f64: a few ulps of the scaled value
    np.testing.assert_allclose(got, want, rtol=2e-6, atol=2e-6)
    np.testing.assert_allclose(got_t, want_t, rtol=2e-6, atol=2e-6)


def test_sklearn_pipelines(api, tmp_path):
    pytest.importorskip("sklearn")
    from sklearn import ensemble, linear_model, svm

    x, y = _sk_data(2000, seed=22)
    ct = _column_transformer(x)
    Fp = _dense(ct.transform(x[:2].astype(np.float64))).shape[1]
    yc = np.digitize(y, np.quantile(y, [0.33, 0.66]))
    # the estimators are fitted on the f32 rows the Prep step produces, so the model and the check see the same features
    _load(api, tmp_path, "ctx", W.sklearn_column_transformer(ct))
    try:
        feats = api.predict("ctx", x)
    finally:
        api.unload_model("ctx")
    cases = []
    rf = ensemble.RandomForestClassifier(n_estimators=20, max_depth=8, random_state=0).fit(feats, yc)
    cases.append(("rf", W.tree_head(W.sklearn_tree_spec(rf, Fp)), rf))
    gb = ensemble.GradientBoostingRegressor(n_estimators=30, max_depth=3, random_state=0).fit(feats, y)
    cases.append(("gb", W.tree_head(W.sklearn_tree_spec(gb, Fp)), gb))
    lr = linear_model.LogisticRegression(max_iter=500).fit(feats, yc)
    cases.append(("lr", W.linear_head(lr.coef_, lr.intercept_, [int(c) for c in lr.classes_]), lr))
    sv = svm.SVC(kernel="rbf", decision_function_shape="ovo").fit(feats, yc)
    cases.append(("svc", W.svm_head(W.sklearn_svm_spec(sv, Fp)), sv))
    for name, head, est in cases:
        _load(api, tmp_path, name, W.sklearn_column_transformer(ct, estimator_graph=head))
        try:
            got = api.predict(name, x).reshape(-1)
        finally:
            api.unload_model(name)
        if name == "gb":
            np.testing.assert_allclose(got, est.predict(feats), rtol=1e-4, atol=1e-5)
            continue
        want = est.predict(feats).astype(f32)
        if name == "rf":
            p = np.sort(est.predict_proba(feats), axis=1)
            decisive = p[:, -1] - p[:, -2] > 1e-4
        elif name == "lr":
            s = np.sort(est.decision_function(feats), axis=1)
            decisive = s[:, -1] - s[:, -2] > 1e-4
        else:
            decisive = np.min(np.abs(est.decision_function(feats)), axis=1) > 1e-3
        print(f"{name}: {int((~decisive).sum())} rows near a tie excluded")
        assert np.array_equal(got[decisive], want[decisive]), name
    # the forest's probabilities through the pipeline's ZipMap output
    blob = W.sklearn_column_transformer(ct, estimator_graph=W.tree_head(W.sklearn_tree_spec(rf, Fp)), zipmap=True)
    _load(api, tmp_path, "rfz", blob, "#output_probability")
    try:
        np.testing.assert_allclose(api.predict("rfz", x), rf.predict_proba(feats), rtol=1e-4, atol=1e-5)
    finally:
        api.unload_model("rfz")
