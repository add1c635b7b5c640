"""TreeEnsembleRegressor / TreeEnsembleClassifier on the GPU (hip/trees.hip) against a float64 numpy restatement of the
ONNX-ML specification written here, and bit-reproducibility across every call path."""
from __future__ import annotations

import numpy as np
import pytest

from infera_amd import onnx_writer as W
from infera_amd import synth

RTOL, ATOL = 1e-4, 1e-6

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api(built):
    from infera_amd import capi

    assert capi.device_count() >= 1, capi.get_devices()
    return capi


# ---- the restatement -----------------------------------------------------------------------------------------------------------

def np_tree_ensemble(spec, x32):
    """(label or None, scores [N, E]) in float64; every decision compares the f32 feature with the threshold as given (f32, or the
    double of a *_as_tensor attribute), under IEEE rules; NaN follows nodes_missing_value_tracks_true."""
    x = x32.astype(np.float64)
    N, E = x.shape[0], spec["E"]
    cls = spec["kind"] == "classifier"
    tid, nid = np.asarray(spec["nodes_treeids"]), np.asarray(spec["nodes_nodeids"])
    index = {(int(t), int(n)): i for i, (t, n) in enumerate(zip(tid, nid))}
    feat = np.asarray(spec["nodes_featureids"])
    modes = spec["nodes_modes"]
    vals = spec["nodes_values"]
    tch = np.array([index.get((int(t), int(c)), -1) for t, c in zip(tid, spec["nodes_truenodeids"])])
    fch = np.array([index.get((int(t), int(c)), -1) for t, c in zip(tid, spec["nodes_falsenodeids"])])
    mtt = np.asarray(spec["nodes_missing_value_tracks_true"]) if spec["missing"] else np.zeros(len(tid), dtype=np.int64)
    is_leaf = np.array([m == "LEAF" for m in modes])
    binary = cls and E == 2 and len(set(spec["leaf_ids"])) == 1
    Wd = 1 if binary else E
    leafv = np.zeros((len(tid), Wd))
    for t, n, j, w in zip(spec["leaf_treeids"], spec["leaf_nodeids"], spec["leaf_ids"], spec["leaf_weights"]):
        leafv[index[(int(t), int(n))], 0 if binary else int(j)] += w
    leafv = leafv.astype(np.float32).astype(np.float64)  # the loader keeps each leaf's summed value as f32
    children = set(int(c) for c in tch[~is_leaf]) | set(int(c) for c in fch[~is_leaf])
    trees = list(dict.fromkeys(int(t) for t in tid))
    roots = {int(tid[i]): i for i in range(len(tid)) if i not in children}
    ops = {"BRANCH_LEQ": np.less_equal, "BRANCH_LT": np.less, "BRANCH_GTE": np.greater_equal, "BRANCH_GT": np.greater,
           "BRANCH_EQ": np.equal, "BRANCH_NEQ": np.not_equal}
    opidx = {m: k for k, m in enumerate(ops)}
    mcode = np.array([opidx.get(m, -1) for m in modes])
    raw = np.zeros((N, Wd))
    rows = np.arange(N)
    for t in trees:
        cur = np.full(N, roots[t])
        while True:
            act = ~is_leaf[cur]
            if not act.any():
                break
            c = cur[act]
            v = x[rows[act], feat[c]]
            th = vals[c]
            res = np.zeros(c.size, dtype=bool)
            for name, k in opidx.items():
                sel = mcode[c] == k
                res[sel] = ops[name](v[sel], th[sel])
            nan = np.isnan(v)
            res = np.where(nan & (mtt[c] != 0), True, res)
            cur[act] = np.where(res, tch[c], fch[c])
        raw += leafv[cur]
    if spec["aggregate"] == "AVERAGE":
        raw /= len(trees)
    if spec["base_values"] is not None:
        raw += spec["base_values"][None, :]
    post = spec["post"]
    label = None
    if binary:
        s = raw[:, 0]
        signed = (np.asarray(spec["leaf_weights"]) < 0).any()
        scores = np.stack([-s, s], 1) if signed else np.stack([1 - s, s], 1)
        if cls:
            label = np.where(s > (0 if signed else 0.5), spec["labels"][1], spec["labels"][0])
    else:
        scores = raw
        if cls:
            label = np.asarray(spec["labels"])[np.argmax(raw, 1)]
    if post == "LOGISTIC":
        scores = 1 / (1 + np.exp(-scores))
    elif post == "SOFTMAX":
        e = np.exp(scores - scores.max(1, keepdims=True))
        scores = e / e.sum(1, keepdims=True)
    return label, scores, raw


def assert_close(got, want):
    assert got.shape == want.shape, (got.shape, want.shape)
    err = np.abs(got.astype(np.float64) - want)
    bad = err > RTOL * np.abs(want) + ATOL
    assert not bad.any(), f"{bad.sum()} / {bad.size} out of tolerance; worst err {err.max():.3e}"


def _table(rows, F, seed=23, nan_frac=0.0):
    x = synth.table(seed, 0, rows, F)
    if nan_frac:
        rng = np.random.default_rng(seed)
        x[rng.random(x.shape) < nan_frac] = np.nan
    return x


def _run(api, tmp_path, spec, x, select="", scaler=None, name="te"):
    p = W.write(str(tmp_path / f"{name}.onnx"), W.tree_ensemble_from_spec(spec, scaler=scaler, output="label"))
    api.load_model(name, p + select)
    try:
        return api.predict(name, x)
    finally:
        api.unload_model(name)


# ---- regressors ----------------------------------------------------------------------------------------------------------------

REG = [  # features, trees, depth, ragged, targets, aggregate, base
    (4, 1, 6, False, 1, "SUM", False),
    (30, 100, 6, False, 1, "SUM", True),
    (30, 50, 8, False, 3, "AVERAGE", True),
    (128, 200, 8, False, 1, "SUM", False),
    (256, 20, 21, True, 3, "SUM", True),
    (561, 30, 20, True, 1, "AVERAGE", False),
    (30, 1000, 6, False, 1, "SUM", True),
    (16, 12, 7, False, 20, "SUM", True),  # walk width above the register buckets: accumulation in the partial buffer
]


@pytest.mark.parametrize("case", REG, ids=lambda c: "F{}_T{}_d{}{}_E{}_{}".format(c[0], c[1], c[2], "r" if c[3] else "", c[4], c[5]))
def test_regressor_vs_numpy(api, tmp_path, case):
    F, T, d, ragged, E, agg, base = case
    x = _table(3001, F)
    spec = W.tree_ensemble_spec(features=F, trees=T, depth=d, ragged=ragged, targets=E, aggregate=agg, base_values=base,
                                thresholds=x[:64], modes=W.TREE_MODES, seed=F + T)
    got = _run(api, tmp_path, spec, x)
    _, want, _ = np_tree_ensemble(spec, x)
    assert_close(got, want)


def test_every_mode_on_threshold_ties_and_nan(api, tmp_path):
    """Thresholds equal to table values (LEQ vs LT and GT vs GTE differ on those rows), NaN features, both missing flags."""
    F = 6
    x = _table(4099, F, seed=5, nan_frac=0.1)
    x[::3] = np.round(x[::3] * 4) / 4  # many exact ties
    pool = np.unique(np.round(x[np.isfinite(x)] * 4) / 4)
    for modes in [(m,) for m in W.TREE_MODES] + [W.TREE_MODES]:
        spec = W.tree_ensemble_spec(features=F, trees=6, depth=7, ragged=False, thresholds=pool, modes=modes, missing=True, seed=len(modes[0]))
        got = _run(api, tmp_path, spec, x)
        _, want, _ = np_tree_ensemble(spec, x)
        assert_close(got, want)


def test_leaf_choice_exact_pow2(api, tmp_path):
    """Distinct powers of two at the leaves: the f32 sum names every leaf reached, so the choice must match exactly."""
    F = 30
    x = _table(5000, F, seed=9, nan_frac=0.02)
    spec = W.tree_ensemble_spec(features=F, trees=3, depth=3, modes=W.TREE_MODES, missing=True, thresholds=x[:40], pow2_leaves=True, seed=2)
    got = _run(api, tmp_path, spec, x)
    _, want, _ = np_tree_ensemble(spec, x)
    assert np.array_equal(got.astype(np.float64), want)


def test_as_tensor_double_thresholds(api, tmp_path):
    """Opset-3 double thresholds a quarter ulp off table values: rounding them to nearest would flip the ties."""
    F = 8
    x = _table(4096, F, seed=11)
    x[::2] = np.round(x[::2] * 8) / 8
    pool = np.unique(np.round(x * 8) / 8)
    spec = W.tree_ensemble_spec(features=F, trees=10, depth=6, as_tensor=True, thresholds=pool, modes=W.TREE_MODES, base_values=True,
                                pow2_leaves=False, seed=12)
    got = _run(api, tmp_path, spec, x)
    _, want, _ = np_tree_ensemble(spec, x)
    assert_close(got, want)
    # the same ensemble with the thresholds rounded to nearest f32 decides differently on some rows: the test can see a flip
    spec_rn = dict(spec, nodes_values=spec["nodes_values"].astype(np.float32).astype(np.float64))
    _, want_rn, _ = np_tree_ensemble(spec_rn, x)
    assert not np.allclose(want_rn, want, rtol=RTOL, atol=ATOL)


def test_scaler_pipeline(api, tmp_path):
    F = 12
    x = _table(3000, F, seed=13)
    off = np.linspace(-0.3, 0.3, F).astype(np.float32)
    sc = np.linspace(0.7, 1.9, F).astype(np.float32)
    # the Scaler runs as the product's one multiply-add per feature, x * scale + f32(-offset * scale) (lowering.cpp folds Sub and Mul
    # into one AffineChannel step); the trees compare THAT f32 value -- nothing is folded into the thresholds
    shift = (-off.astype(np.float64) * sc).astype(np.float32)
    xs = (x.astype(np.float64) * sc + shift).astype(np.float32)
    spec = W.tree_ensemble_spec(features=F, trees=40, depth=6, thresholds=xs[:50], modes=W.TREE_MODES, base_values=True, seed=14)
    got = _run(api, tmp_path, spec, x, scaler=(off, sc))
    _, want, _ = np_tree_ensemble(spec, xs)
    assert_close(got, want)


# ---- classifiers ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("post", ["NONE", "LOGISTIC", "SOFTMAX"])
def test_classifier_labels_and_scores(api, tmp_path, post):
    F = 30
    x = _table(4000, F, seed=17)
    spec = W.tree_ensemble_spec(features=F, trees=60, depth=12, ragged=True, kind="classifier", labels=[3, 7, 42], post=post,
                                modes=W.TREE_MODES, base_values=True, thresholds=x[:60], seed=18)
    label = _run(api, tmp_path, spec, x).reshape(-1)
    scores = _run(api, tmp_path, spec, x, select="#probabilities")
    want_label, want_scores, raw = np_tree_ensemble(spec, x)
    assert_close(scores, want_scores)
    top2 = np.sort(raw, 1)[:, -2:]
    decisive = (top2[:, 1] - top2[:, 0]) > 1e-4 * np.abs(top2[:, 1]) + 1e-5
    assert decisive.sum() > 3500
    assert set(np.unique(label)) <= {3.0, 7.0, 42.0}
    assert np.array_equal(label[decisive], want_label[decisive].astype(np.float32))


@pytest.mark.parametrize("binary,post", [("signed", "NONE"), ("signed", "LOGISTIC"), ("positive", "NONE")])
def test_binary_single_column(api, tmp_path, binary, post):
    F = 30
    x = _table(4000, F, seed=19)
    spec = W.tree_ensemble_spec(features=F, trees=50, depth=6, kind="classifier", labels=[0, 5], binary=binary, post=post,
                                base_values=True, thresholds=x[:60], seed=20)
    label = _run(api, tmp_path, spec, x).reshape(-1)
    scores = _run(api, tmp_path, spec, x, select="#probabilities")
    want_label, want_scores, raw = np_tree_ensemble(spec, x)
    assert_close(scores, want_scores)
    cut = 0.0 if binary == "signed" else 0.5
    decisive = np.abs(raw[:, 0] - cut) > 1e-4
    assert np.array_equal(label[decisive], want_label[decisive].astype(np.float32))


# ---- reproducibility -----------------------------------------------------------------------------------------------------------

def test_bits_independent_of_call_path(api, tmp_path):
    from infera_amd import sqlharness

    F, rows = 30, 100_000
    x = _table(rows, F, seed=29)
    spec = W.tree_ensemble_spec(features=F, trees=100, depth=6, thresholds=x[:64], modes=W.TREE_MODES, base_values=True, seed=30)
    p = W.write(str(tmp_path / "rep.onnx"), W.tree_ensemble_from_spec(spec))
    api.load_model("rep", p)
    try:
        ref = api.predict("rep", x)
        for step in (1, 7, 2048, 2049):
            n = rows if step > 1 else 5000  # (one row per call: the first 5000 rows)
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
        sqlharness.sql("infera_load_model", "rep_sql", p)
        try:
            got = sqlharness.sql("infera_predict", "rep_sql", *[np.ascontiguousarray(x[4096:6144, j]) for j in range(F)])
        finally:
            sqlharness.sql("infera_unload_model", "rep_sql")
        assert np.array_equal(np.asarray(got, dtype=np.float32), ref[4096:6144, 0])
    finally:
        api.unload_model("rep")
    _, want, _ = np_tree_ensemble(spec, x[:5000])
    assert_close(ref[:5000], want)


def test_device_resident_matches_host(api, tmp_path):
    F, rows = 128, 20_000
    x = _table(rows, F, seed=31)
    spec = W.tree_ensemble_spec(features=F, trees=64, depth=8, thresholds=x[:64], seed=32)
    p = W.write(str(tmp_path / "dev.onnx"), W.tree_ensemble_from_spec(spec))
    api.load_model("dev", p)
    try:
        ref = api.predict("dev", x)
        for d in range(api.device_count()):
            dev = api.device_ordinal(d)
            d_in = api.DeviceBuffer(dev, x.nbytes)
            d_out = api.DeviceBuffer(dev, rows * 4)
            d_in.upload(x)
            api.predict_device("dev", d_in, rows, F, d_out)
            assert np.array_equal(d_out.download((rows, 1)), ref), f"device slot {d}"
    finally:
        api.unload_model("dev")


# ---- optional: sklearn models written through the builder ----------------------------------------------------------------------

def _sk_spec(est_trees, F, kind, E, scale=1.0, labels=None):
    nodes = {k: [] for k in ("nodes_treeids", "nodes_nodeids", "nodes_featureids", "nodes_modes", "nodes_values", "nodes_truenodeids",
                             "nodes_falsenodeids")}
    lt, ln, lid, lw = [], [], [], []
    for t, tr in enumerate(est_trees):
        for i in range(tr.node_count):
            leaf = tr.children_left[i] < 0
            nodes["nodes_treeids"].append(t)
            nodes["nodes_nodeids"].append(i)
            nodes["nodes_featureids"].append(0 if leaf else int(tr.feature[i]))
            nodes["nodes_modes"].append("LEAF" if leaf else "BRANCH_LEQ")
            nodes["nodes_values"].append(0.0 if leaf else float(tr.threshold[i]))
            nodes["nodes_truenodeids"].append(0 if leaf else int(tr.children_left[i]))
            nodes["nodes_falsenodeids"].append(0 if leaf else int(tr.children_right[i]))
            if leaf:
                v = tr.value[i].ravel()
                if kind == "classifier":
                    v = v / v.sum()
                for j in range(E):
                    lt.append(t), ln.append(i), lid.append(j), lw.append(float(v[j]) * scale)
    spec = {"kind": kind, "features": F, "E": E, "labels": labels or list(range(E)), "aggregate": "SUM", "post": "NONE",
            "as_tensor": True, "missing": False, "nodes_missing_value_tracks_true": [0] * len(nodes["nodes_treeids"]),
            "leaf_treeids": lt, "leaf_nodeids": ln, "leaf_ids": lid, "leaf_weights": np.array(lw), "base_values": None}
    spec.update(nodes)
    spec["nodes_values"] = np.array(spec["nodes_values"])
    return spec


def _between(x, spec):
    """rows where some feature lies between a double threshold and its f32 rounding (sklearn compares f32 x with the double)"""
    bad = np.zeros(x.shape[0], dtype=bool)
    for f, m, t in zip(spec["nodes_featureids"], spec["nodes_modes"], spec["nodes_values"]):
        if m == "LEAF":
            continue
        lo, hi = sorted((t, float(np.float32(t))))
        bad |= (x[:, f] >= lo) & (x[:, f] <= hi)
    return bad


def test_sklearn_cross_check(api, tmp_path):
    ens = pytest.importorskip("sklearn.ensemble")
    F = 10
    x = _table(3000, F, seed=41)
    y = (np.sin(3 * x[:, 0]) + x[:, 1] * x[:, 2]).astype(np.float32)
    gb = ens.GradientBoostingRegressor(n_estimators=30, max_depth=4, random_state=0).fit(x, y)
    spec = _sk_spec([e[0].tree_ for e in gb.estimators_], F, "regressor", 1, scale=gb.learning_rate)
    spec["base_values"] = np.array([float(gb.init_.constant_.ravel()[0])])
    got = _run(api, tmp_path, spec, x, name="gb")[:, 0]
    keep = ~_between(x, spec)
    print(f"GradientBoostingRegressor: {int((~keep).sum())} rows excluded (a feature between a threshold and its f32 rounding)")
    np.testing.assert_allclose(got[keep], gb.predict(x)[keep], rtol=1e-4, atol=1e-5)

    yc = np.digitize(y, np.quantile(y, [0.33, 0.66]))
    rf = ens.RandomForestClassifier(n_estimators=20, max_depth=12, random_state=0).fit(x, yc)
    spec = _sk_spec([e.tree_ for e in rf.estimators_], F, "classifier", 3)
    spec["aggregate"] = "AVERAGE"
    got = _run(api, tmp_path, spec, x, select="#probabilities", name="rf")
    keep = ~_between(x, spec)
    print(f"RandomForestClassifier: {int((~keep).sum())} rows excluded")
    np.testing.assert_allclose(got[keep], rf.predict_proba(x)[keep], rtol=1e-4, atol=1e-5)
