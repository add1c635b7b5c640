"""The k-NN vote (hip/nearest.hip nearest_vote_kernel) on the GPU against tests/knn_vote_ref.py (the contract: INTEGRATION.md section 2.6
"The k-NN vote").  On integer grids every distance is exact, so the label, the probabilities and the regression value must equal the f32
restatement BIT FOR BIT in every graph form.  With distance weights the neighbours come from the SEARCH model of the same spec and the
results lie within the rounding budget of the float64 evaluation.  On generic data a row whose (k + 1)-th neighbour lies within twice the
distance bound of the k-th is excluded (<= 1 %; the share is asserted from the reference alone in tests/test_knn_vote.py)."""
from __future__ import annotations

import numpy as np
import pytest

from infera_amd import onnx_writer as W
from tests import knn_vote_ref as R
from tests.test_knn_vote import GENERIC, excluded_rows, generic_case

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
GRID_CAP = 4096  # blocks of 64 rows (hip/nearest.hip kVoteGridCap)


@pytest.fixture(scope="module")
def api(built):
    from infera_amd import capi

    assert capi.device_count() >= 1, capi.get_devices()
    return capi


_n = [0]


def _predict(api, tmp_path, blob, xs, select=""):
    """the served output for each row matrix of `xs`, from one load"""
    _n[0] += 1
    name = f"kv{_n[0]}"
    p = W.write(str(tmp_path / f"{name}.onnx"), blob)
    api.load_model(name, p + select)
    try:
        return [api.predict(name, x) for x in xs]
    finally:
        api.unload_model(name)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(got, want):
    return got.size == want.size and np.array_equal(bits(got).reshape(-1), bits(want).reshape(-1))


# ---- exact grids -----------------------------------------------------------------------------------------------------------------

def _grid_set(F, M, seed):
    """integers in [-8, 8]: +- pairs around an integer shift vector (and the shift itself when M is odd), so the mean is that vector
    (the construction of tests/test_nearest_gpu.py)"""
    rng = np.random.default_rng(seed)
    shift = rng.integers(-3, 4, F) if seed % 2 else np.zeros(F, np.int64)
    half = rng.integers(-5, 6, (M // 2, F))
    c = np.concatenate([shift + half, shift - half] + ([shift[None, :]] if M % 2 else []))
    return {"features": F, "centers": c[rng.permutation(M)].astype(np.float32)}


ROWS = (1, 31, 33, 64, 65, 129)


def _labels(rng, M, C):
    """class indices of the M training rows; from 3 classes on, class C // 2 is carried by no row"""
    pool = np.array([c for c in range(C) if C < 3 or c != C // 2])
    return pool[rng.integers(0, len(pool), M)]


def _class_values(C):
    return [3, 7, 8, 20, 21, 50, 64][:C]  # (not evenly spaced)


@pytest.mark.parametrize("M", [2, 33, 100, 600])
@pytest.mark.parametrize("F", [1, 8, 36])
def test_exact_grids(api, tmp_path, F, M):
    spec = _grid_set(F, M, F + M)
    rng = np.random.default_rng(F * 1000 + M)
    x = rng.integers(-8, 9, (ROWS[-1], F)).astype(np.float32)
    xs = [x[:r] for r in ROWS]
    ks = sorted({k for k in (1, 2, 5, 16, M) if k <= min(M, 16)})
    refs = {k: W.nearest_reference(spec, x, k) for k in ks}
    assert refs[ks[0]]["d2"].max() < 2 ** 24
    target = rng.integers(-64, 65, M)
    ys = {C: _labels(rng, M, C) for C in (2, 3, 7)}

    def check(got, want, what):
        for r, g in zip(ROWS, got):
            assert same_bits(g, want[:r]), (what, r)

    def classifier(k, C, weights="uniform", **form):
        f = R.vote_f32(refs[k]["indices"], refs[k]["values"], y=ys[C], C=C, weights=weights, rooted=form.get("spelling", "cdist") == "cdist" or weights == "distance")
        cv = np.array(_class_values(C), np.float32)
        check(_predict(api, tmp_path, W.knn_classifier_from_spec(spec, ys[C], _class_values(C), k, weights, "label", **form), xs), cv[f["label"]], ("label", k, C, weights, form))
        check(_predict(api, tmp_path, W.knn_classifier_from_spec(spec, ys[C], _class_values(C), k, weights, "probabilities", **form), xs), f["proba"], ("proba", k, C, weights, form))
        assert (f["proba"][:, C // 2] == 0).all() or C < 3

    def regressor(k, weights="uniform", **form):
        f = R.vote_f32(refs[k]["indices"], refs[k]["values"], target=target, weights=weights, rooted=form.get("spelling", "cdist") == "cdist" or weights == "distance")
        check(_predict(api, tmp_path, W.knn_regressor_from_spec(spec, target, k, weights, **form), xs), f["value"], ("value", k, weights, form))

    for k in ks:
        for C in (2, 3, 7):
            classifier(k, C)
        regressor(k)
    k0 = ks[min(2, len(ks) - 1)]
    for spelling in W.NEAREST_SPELLINGS:  # every spelling, both lookups, both keepdims forms
        for lookup in ("afe", "gather"):
            for keepdims in (1, 0):
                classifier(k0, 3, spelling=spelling, lookup=lookup, keepdims=keepdims)
                regressor(k0, spelling=spelling, lookup=lookup, keepdims=keepdims)
    classifier(k0, 7, keepdims=0, join="transpose")
    # beyond what is asked: on exact distances the distance weights are exact operations too (sqrt, max, one division), rows that coincide
    # with a training point (d = 0, F = 1 has them for sure) included -- the same bits
    classifier(k0, 3, weights="distance")
    classifier(k0, 7, weights="distance", spelling="gemm")
    regressor(k0, weights="distance")
    if F == 1:
        assert (refs[k0]["values"][:, 0] == 0).any()
    if M == 600:  # (several slices: the merge runs)
        p = W.write(str(tmp_path / "plan.onnx"), W.knn_regressor_from_spec(spec, target, k0))
        api.load_model("kv_plan", p)
        try:
            assert api.get_plan("kv_plan")["plan"]["steps"][1]["slices"] >= 2
        finally:
            api.unload_model("kv_plan")


@pytest.mark.parametrize("C", [65, 256])
def test_probability_store_path(api, tmp_path, C):
    """more classes than lanes, and the cap: rows of C floats leave the wave through LDS; the columns no neighbour touches are exactly 0"""
    F, M, k = 8, 100, 16
    spec = _grid_set(F, M, 5)
    rng = np.random.default_rng(C)
    x = rng.integers(-8, 9, (65, F)).astype(np.float32)
    y = rng.integers(0, C, M)
    ref = W.nearest_reference(spec, x, k)
    f = R.vote_f32(ref["indices"], ref["values"], y=y, C=C)
    got = _predict(api, tmp_path, W.knn_classifier_from_spec(spec, y, list(range(C)), k, output="probabilities"), [x[:1], x[:63], x])
    for g, r in zip(got, (1, 63, 65)):
        assert g.shape == (r, C) and same_bits(g, f["proba"][:r]), r
        touched = np.zeros((r, C), bool)
        np.put_along_axis(touched, y[ref["indices"][:r]], True, 1)
        assert (bits(g)[~touched] == 0).all() and (g[touched] > 0).all()
    lab = _predict(api, tmp_path, W.knn_classifier_from_spec(spec, y, list(range(C)), k), [x])[0]
    assert same_bits(lab, f["label"].astype(np.float32))


def test_grid_stride(api, tmp_path):
    """more 64-row tiles than the grid has blocks: a block walks on with the grid's stride"""
    rows = GRID_CAP * 64 + 65
    spec = {"features": 1, "centers": np.array([[-1.0], [2.0]], np.float32)}
    x = np.random.default_rng(3).integers(-8, 9, (rows, 1)).astype(np.float32)
    got = _predict(api, tmp_path, W.knn_classifier_from_spec(spec, np.array([1, 0]), [4, 9], 1), [x])[0].reshape(-1)
    want = np.where(np.abs(x[:, 0] + 1) <= np.abs(x[:, 0] - 2), 9.0, 4.0).astype(np.float32)  # (x = 0.5 does not occur: no ties)
    assert got.shape == (rows,) and np.array_equal(got, want)


# ---- distance weights ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("spelling", ["cdist", "gemm"])
def test_distance_weights(api, tmp_path, spelling):
    """the neighbours and their distances come from the search model of the same spec (it does not run the vote); probabilities within
    (2 k + 2) 2^-24 p_c of the float64 evaluation (one rounding for w, k - 1 adds in each of v_c and s, one division), the value within
    (k + 2) 2^-24 sum |w t| / sum w; the label is the float64 label unless the two largest class weights are within twice that bound"""
    F, M, k, C, eps = 30, 600, 5, 4, 0.05
    spec, x, y, t = generic_case(F, M, 11, k, C)
    x = np.concatenate([x, spec["centers"][7:8]])  # a row that coincides with a training point: the eps clamp decides its first weight
    idx = _predict(api, tmp_path, W.knn_search_from_spec(spec, k, "indices", spelling), [x])[0].astype(np.int64)
    dist = _predict(api, tmp_path, W.knn_search_from_spec(spec, k, "distances", spelling), [x])[0].astype(np.float64)
    assert idx[-1, 0] == 7 and dist[-1, 0] < eps < dist[-1, 1] and (dist[:-1] > eps).all()
    want = R.vote_reference(idx, dist, y=y, target=t, C=C, weights="distance", eps=eps)
    assert want["w"][-1, 0] == 1 / np.float64(np.float32(eps))
    form = dict(spelling=spelling, eps=eps)
    proba = _predict(api, tmp_path, W.knn_classifier_from_spec(spec, y, _class_values(C), k, "distance", "probabilities", **form), [x])[0].astype(np.float64)
    pb = (2 * k + 2) * U * want["proba"]
    print(f"{spelling}: worst probability error / bound = {np.nanmax(np.abs(proba - want['proba'])[pb > 0] / pb[pb > 0]):.3f}")
    assert (np.abs(proba - want["proba"]) <= pb).all()
    value = _predict(api, tmp_path, W.knn_regressor_from_spec(spec, t, k, "distance", **form), [x])[0].reshape(-1).astype(np.float64)
    vb = (k + 2) * U * want["mag"]
    print(f"{spelling}: worst value error / bound = {(np.abs(value - want['value']) / np.maximum(vb, 1e-300)).max():.3f}")
    assert (np.abs(value - want["value"]) <= vb).all()
    label = _predict(api, tmp_path, W.knn_classifier_from_spec(spec, y, _class_values(C), k, "distance", "label", **form), [x])[0].reshape(-1)
    top = np.sort(want["proba"], 1)
    excluded = top[:, -1] - top[:, -2] < 2 * (2 * k + 2) * U * top[:, -1]
    print(f"{spelling}: {int(excluded.sum())} of {x.shape[0]} rows excluded")
    assert excluded.mean() <= 0.01
    assert np.array_equal(label[~excluded], np.array(_class_values(C), np.float32)[want["label"]][~excluded])


# ---- generic data ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("F,M,seed,k", GENERIC)
def test_generic_uniform(api, tmp_path, F, M, seed, k):
    """uniform weights against the float64 neighbour SETS: where the set is decided (the file's convention on gap_out), counts and sums of
    whole-number targets do not depend on the order inside it, so the bits are the restatement's"""
    C = 4
    spec, x, y, t = generic_case(F, M, seed, k, C)
    ref = W.nearest_reference(spec, x, k)
    keep = ~excluded_rows(spec, x, k)
    print(f"{int((~keep).sum())} of {x.shape[0]} rows excluded")
    assert (~keep).mean() <= 0.01
    f = R.vote_f32(ref["indices"], ref["values"], y=y, target=t, C=C)
    cv = np.array(_class_values(C), np.float32)
    for spelling in (W.NEAREST_SPELLINGS if F == 30 else ("cdist",)):
        label = _predict(api, tmp_path, W.knn_classifier_from_spec(spec, y, _class_values(C), k, spelling=spelling), [x])[0].reshape(-1)
        assert same_bits(label[keep], cv[f["label"]][keep]), spelling
        proba = _predict(api, tmp_path, W.knn_classifier_from_spec(spec, y, _class_values(C), k, output="probabilities", spelling=spelling), [x])[0]
        assert same_bits(proba[keep], f["proba"][keep]), spelling
        value = _predict(api, tmp_path, W.knn_regressor_from_spec(spec, t, k, spelling=spelling), [x])[0].reshape(-1)
        assert same_bits(value[keep], f["value"][keep]), spelling


# ---- NaN rows and call paths -----------------------------------------------------------------------------------------------------

def test_nan_row_and_chunking(api, tmp_path):
    """a NaN row ranks its neighbours by index (0 .. k - 1): uniform weights give it the vote of those labels, distance weights NaN
    probabilities, a NaN value and -- the ArgMax step's rule: element 0 starts the scan, NaN never compares greater -- the label of class
    0.  It poisons only itself; one call and calls of 1 / 33 rows give the same bits"""
    F, M, k, C = 30, 600, 5, 4
    spec, x, y, t = generic_case(F, M, 11, k, C)
    x = x[:130].copy()
    clean = x.copy()
    x[17, 3] = np.nan
    others = np.arange(130) != 17
    first = np.arange(k)[None, :]
    cv = np.array(_class_values(C), np.float32)
    for weights in ("uniform", "distance"):
        nan_f = R.vote_f32(first, np.full((1, k), np.nan, np.float32), y=y, target=t, C=C, weights=weights)
        for kind, blob in (("label", W.knn_classifier_from_spec(spec, y, _class_values(C), k, weights)),
                           ("proba", W.knn_classifier_from_spec(spec, y, _class_values(C), k, weights, "probabilities")),
                           ("value", W.knn_regressor_from_spec(spec, t, k, weights))):
            p = W.write(str(tmp_path / f"nan_{weights}_{kind}.onnx"), blob)
            api.load_model("kv_nan", p)
            try:
                got = api.predict("kv_nan", x)
                ref = api.predict("kv_nan", clean)
                got, ref = got.reshape(130, -1), ref.reshape(130, -1)
                assert same_bits(got[others], ref[others]) and not np.isnan(ref).any(), (weights, kind)
                want = {"label": cv[nan_f["label"]], "proba": nan_f["proba"], "value": nan_f["value"]}[kind]
                assert np.array_equal(got[17], np.asarray(want, np.float32).reshape(-1), equal_nan=True), (weights, kind, got[17])
                if weights == "distance":
                    assert got[17, 0] == cv[0] if kind == "label" else np.isnan(got[17]).all()
                for step in (1, 33):
                    parts = np.concatenate([api.predict("kv_nan", x[i:i + step]).reshape(-1, got.shape[1]) for i in range(0, 130 if step > 1 else 40, step)])
                    assert same_bits(parts, got[:parts.shape[0]]), (weights, kind, step)
            finally:
                api.unload_model("kv_nan")
