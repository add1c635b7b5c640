"""Distance models (hip/nearest.hip) and the feature-axis reductions (hip/reduce.hip) on the GPU against float64 numpy restatements
(onnx_writer.nearest_reference / reduce_reference; the contract: INTEGRATION.md section 2.6).  On integer grids every f32 value is exact,
so the fused step, the operator-by-operator plan (INFERA_NEAREST=0), all spellings and the reference must agree BIT FOR BIT.  On generic
data every distance lies within TOL and a row whose deciding float64 gap is below 2 TOL is excluded (<= 1 %)."""
from __future__ import annotations

import numpy as np
import pytest

from infera_amd import onnx_writer as W

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


@pytest.fixture(scope="module")
def api(built):
    from infera_amd import capi

    assert capi.device_count() >= 1, capi.get_devices()
    return capi


_n = [0]


def _predict(api, tmp_path, blob, xs, select=""):
    """the served output for each row matrix of `xs`, from one load"""
    _n[0] += 1
    name = f"nn{_n[0]}"
    p = W.write(str(tmp_path / f"{name}.onnx"), blob)
    api.load_model(name, p + select)
    try:
        return [api.predict(name, x) for x in xs]
    finally:
        api.unload_model(name)


def tol_of(ref, F):
    """|served d2 - d2| <= (F + 12) 2^-24 mag: F_pad + 4 <= F + 11 roundings of relative size 2^-24, each on a partial result bounded by
    mag, + 1 for the second-order terms"""
    return (F + 12) * U * ref["mag"]


def sqrt_tol(tol, d2):
    with np.errstate(all="ignore"):
        return np.minimum(np.where(d2 > 0, tol / np.sqrt(d2), np.inf), np.sqrt(tol)) + 2 * U * np.sqrt(d2)


# ---- exact grids -----------------------------------------------------------------------------------------------------------------

def _grid_set(F, M, seed):
    """integers in [-8, 8]: +- pairs around an integer shift vector (and the shift itself when M is odd), so the mean is that vector"""
    rng = np.random.default_rng(seed)
    shift = rng.integers(-3, 4, F) if seed % 2 else np.zeros(F, np.int64)
    half = rng.integers(-5, 6, (M // 2, F))
    c = np.concatenate([shift + half, shift - half] + ([shift[None, :]] if M % 2 else []))
    return {"features": F, "centers": c[rng.permutation(M)].astype(np.float32)}


ROWS = (1, 31, 33, 129)


@pytest.mark.parametrize("M", [1, 2, 31, 32, 33, 100])
@pytest.mark.parametrize("F", [1, 3, 8, 30, 36, 128])
def test_exact_grids(api, tmp_path, monkeypatch, F, M):
    spec = _grid_set(F, M, F + M)
    x = np.random.default_rng(F * 1000 + M).integers(-8, 9, (ROWS[-1], F)).astype(np.float32)
    xs = [x[:r] for r in ROWS]
    ks = sorted({k for k in (1, 5, 16, M) if k <= min(M, 16)})
    refs = {k: W.nearest_reference(spec, x, k) for k in ks}
    d2 = refs[ks[0]]["d2"]
    assert d2.max() < 2 ** 24
    want = {"label": refs[ks[0]]["label"].astype(np.float32), "d2": d2.astype(np.float32), "scores": np.sqrt(d2).astype(np.float32)}

    def check(got, w, what):
        for r, g in zip(ROWS, got):
            assert np.array_equal(g.reshape(w[:r].shape), w[:r]), (what, r)

    k0 = ks[min(1, len(ks) - 1)]
    for sp in W.NEAREST_SPELLINGS + ("generic",):
        if sp == "generic":
            monkeypatch.setenv("INFERA_NEAREST", "0")
        s = "gemm" if sp == "generic" else sp
        for out in ("label", "scores", "d2"):
            check(_predict(api, tmp_path, W.kmeans_from_spec(spec, s, out), xs), want[out], (sp, out))
        for k in (ks if sp == "cdist" else [k0]):
            for metric in ("sqeuclidean", "euclidean"):
                v = refs[k]["values"]
                check(_predict(api, tmp_path, W.knn_search_from_spec(spec, k, "indices", s, metric), xs), refs[k]["indices"].astype(np.float32), (sp, k, "i"))
                check(_predict(api, tmp_path, W.knn_search_from_spec(spec, k, "distances", s, metric), xs),
                      (np.sqrt(v) if metric == "euclidean" else v).astype(np.float32), (sp, k, metric))
    monkeypatch.delenv("INFERA_NEAREST")


def test_ties_lower_index_wins(api, tmp_path):
    """duplicates inside a tile (5, 6), across a tile (5, 37), across a slice boundary; a row equidistant to two distinct vectors"""
    F, M = 6, 600
    rng = np.random.default_rng(7)
    base = rng.integers(-5, 6, (M // 2, F))
    c = np.concatenate([base, -base]).astype(np.float32)  # vector i + M / 2 = -vector i: the mean stays exactly 0
    spec = {"features": F, "centers": c}
    p = W.write(str(tmp_path / "t.onnx"), W.knn_search_from_spec(spec, 16, "indices"))
    api.load_model("ties_plan", p)
    try:
        st = [s for s in api.get_plan("ties_plan")["plan"]["steps"] if s["kind"] == "Nearest"][0]["nearest"]
    finally:
        api.unload_model("ties_plan")
    assert st["slices"] >= 2
    b = 32 * st["slice_tile"][1]  # the first vector of slice 1
    assert 64 < b < M // 2 - 1

    def put(i, v):
        c[i], c[i + M // 2] = v, -v

    v0, v1, w = np.full(F, 40, np.float32), np.full(F, -30, np.float32), np.array([30, -30, 30, -30, 30, -30], np.float32)
    e0 = np.array([1, 0, 0, 0, 0, 0], np.float32)
    for i in (5, 6, 37):
        put(i, v0)
    for i in (b - 1, b):
        put(i, v1)
    put(100, w)
    put(250, w + 2 * e0)
    x = np.stack([v0 + 1, v1 - e0, w + e0, c[3] + e0, -c[9]]).astype(np.float32)
    ref = W.nearest_reference(spec, x, 16)
    assert list(ref["indices"][0][:3]) == [5, 6, 37] and list(ref["indices"][1][:2]) == [b - 1, b] and list(ref["indices"][2][:2]) == [100, 250]
    assert ref["values"][2][0] == ref["values"][2][1] == 1
    for sp in W.NEAREST_SPELLINGS:
        idx = _predict(api, tmp_path, W.knn_search_from_spec(spec, 16, "indices", sp), [x])[0]
        assert np.array_equal(idx, ref["indices"].astype(np.float32)), sp
        lab = _predict(api, tmp_path, W.kmeans_from_spec(spec, sp, "label"), [x])[0]
        assert np.array_equal(lab.reshape(-1), ref["label"].astype(np.float32)), sp


def test_readers_between_the_distances_and_their_consumer(api, tmp_path):
    """Identity / Flatten / Reshape / Dropout between D2 (or Sqrt(D2)) and what consumes it: the same bits as the direct graphs"""
    spec = _grid_set(8, 40, 3)
    x = np.random.default_rng(4).integers(-8, 9, (33, 8)).astype(np.float32)
    ref = W.nearest_reference(spec, x, 1)
    d2, am = ref["d2"].astype(np.float32), [W.attr_i("axis", 1), W.attr_i("keepdims", 0)]
    shape = np.array([0, -1], np.int64)
    cases = [([("Identity", [])], d2), ([("Sqrt", []), ("Identity", [])], np.sqrt(d2)), ([("Identity", []), ("ArgMin", am)], ref["label"].astype(np.float32)),
             ([("Flatten", []), ("Relu", [])], d2), ([("Reshape", [], shape)], d2), ([("Sqrt", []), ("Reshape", [], shape), ("Neg", [])], -np.sqrt(d2)),
             ([("Dropout", []), ("ArgMin", am)], ref["label"].astype(np.float32))]
    for sp in ("gemm", "cdist"):
        for readers, want in cases:
            got = _predict(api, tmp_path, W.distance_reader_graph(spec, readers, sp), [x])[0]
            assert np.array_equal(got.reshape(want.shape), want), (sp, [r[0] for r in readers])


# ---- generic data ----------------------------------------------------------------------------------------------------------------

def _check_generic(api, tmp_path, spec, x, k, spellings=("cdist",), est=None):
    F = spec["features"]
    ref, ref1 = W.nearest_reference(spec, x, k), W.nearest_reference(spec, x, 1)
    tol = tol_of(ref, F)
    nan = np.isnan(x).any(1)
    for sp in spellings:
        d2 = _predict(api, tmp_path, W.kmeans_from_spec(spec, sp, "d2"), [x])[0].astype(np.float64)
        err = np.abs(d2 - ref["d2"])[~nan]
        print(f"{sp}: worst d2 error / TOL = {(err / tol[~nan]).max():.3f}")
        assert (err <= tol[~nan]).all()
        assert np.isnan(d2[nan]).all()
        sc = _predict(api, tmp_path, W.kmeans_from_spec(spec, sp, "scores"), [x])[0].astype(np.float64)
        assert (np.abs(sc - np.sqrt(ref["d2"]))[~nan] <= sqrt_tol(tol, ref["d2"])[~nan]).all()
        # a row is decided by the gaps between its k + 1 nearest; its bound is the largest TOL among them
        near = np.argsort(np.where(np.isnan(ref["d2"]), np.inf, ref["d2"]), 1, kind="stable")[:, :k + 1]
        bound = np.take_along_axis(tol, near, 1).max(1)
        lab = _predict(api, tmp_path, W.kmeans_from_spec(spec, sp, "label"), [x])[0].reshape(-1)
        ex1 = (ref1["gap_out"] < 2 * bound) & ~nan
        exk = (np.minimum(ref["gap_out"], ref["gap_in"]) < 2 * bound) & ~nan
        print(f"{sp}: {int(ex1.sum())} (label) / {int(exk.sum())} (top {k}) of {x.shape[0]} rows excluded")
        assert ex1.mean() <= 0.01 and exk.mean() <= 0.01
        want_lab = ref["label"] if est is None else est[0]
        assert np.array_equal(lab[~ex1 & ~nan], want_lab[~ex1 & ~nan].astype(np.float32))
        assert (lab[nan] == 0).all()  # every distance NaN: ranked by index
        idx = _predict(api, tmp_path, W.knn_search_from_spec(spec, k, "indices", sp), [x])[0]
        want_idx = ref["indices"] if est is None or est[1] is None else est[1]
        keep = ~exk & ~nan
        assert np.array_equal(idx[keep], want_idx[keep].astype(np.float32))
        assert np.array_equal(idx[nan], np.tile(np.arange(k, dtype=np.float32), (int(nan.sum()), 1)))
        val = _predict(api, tmp_path, W.knn_search_from_spec(spec, k, "distances", sp, "sqeuclidean"), [x])[0].astype(np.float64)
        assert (np.abs(val - ref["values"])[~nan] <= bound[~nan, None]).all() and np.isnan(val[nan]).all()


# seeds picked on the CPU from the float64 reference alone (the excluded share stays under the cap)
@pytest.mark.parametrize("F,M,rows,seed", [(30, 100, 200, 2), (128, 1000, 33, 4)])
def test_generic_gaussian(api, tmp_path, F, M, rows, seed):
    spec = W.kmeans_spec(F, M, seed=seed)
    x = np.random.default_rng(seed + 100).standard_normal((rows, F)).astype(np.float32)
    _check_generic(api, tmp_path, spec, x, 10, spellings=W.NEAREST_SPELLINGS if F == 30 else ("cdist",))


@pytest.mark.parametrize("F,seed", [(3, 2), (30, 2)])
def test_offset_data_and_nan_row(api, tmp_path, F, seed):
    """columns of 1000 +- 1: the graph's own f32 arithmetic (|x|^2 ~ 1e6 F) would lose the distances; one NaN row"""
    rng = np.random.default_rng(seed)
    spec = {"features": F, "centers": (1000 + rng.uniform(-1, 1, (40, F))).astype(np.float32)}
    x = (1000 + rng.uniform(-1, 1, (100, F))).astype(np.float32)
    x[17, F // 2] = np.nan
    ref = W.nearest_reference(spec, x, 1)
    assert np.nanmax(tol_of(ref, F) / np.maximum(ref["d2"], 1e-3)) < 0.05  # the centred bound is tight where 2^-24 |x|^2 F ~ 2 is not
    _check_generic(api, tmp_path, spec, x, 5, spellings=("gemm", "cdist"))


def test_sklearn_estimators(api, tmp_path):
    cluster = pytest.importorskip("sklearn.cluster")
    from sklearn.datasets import make_blobs
    from sklearn.neighbors import NearestNeighbors

    x, _ = make_blobs(n_samples=300, n_features=6, centers=8, random_state=3)
    x = x.astype(np.float32)
    km = cluster.KMeans(8, n_init=2, random_state=0).fit(x)
    spec = W.sklearn_kmeans_spec(km)
    nn = NearestNeighbors(n_neighbors=5).fit(x[:150])
    nspec = W.sklearn_neighbors_spec(nn)
    q = x[150:]
    _check_generic(api, tmp_path, spec, q, 5, est=(km.predict(q), None))
    _check_generic(api, tmp_path, nspec, q, 5, est=(nn.kneighbors(q, 1)[1][:, 0], nn.kneighbors(q)[1]))


# ---- reductions ------------------------------------------------------------------------------------------------------------------

EXACT = ("r_ReduceSum", "r_ReduceMax", "r_ReduceMin", "r_ReduceL1", "r_ReduceSumSquare")


@pytest.mark.parametrize("rows", [1, 65])
@pytest.mark.parametrize("F", [1, 5, 64, 1000])
def test_reduce_zoo(api, tmp_path, F, rows):
    rng = np.random.default_rng(F + rows)
    k = min(F, 16)
    xi = rng.integers(-8, 9, (rows, F)).astype(np.float32)  # ties everywhere
    xg = rng.uniform(0.5, 1.5, (rows, F)).astype(np.float32) * np.where(rng.random((rows, F)) < 0.3, -1, 1).astype(np.float32)
    xp = np.abs(xg)
    for keepdims in (1, 0):
        blob, names = W.reduce_zoo(2, F, keepdims=keepdims, k=k, axes_input=bool(keepdims))
        ref = W.reduce_reference(xi, k)
        for nm in names:
            if not (nm in EXACT or nm[0] in "bat") or (keepdims == 0 and nm[0] != "r"):
                continue
            got = _predict(api, tmp_path, blob, [xi], "#" + nm)[0]
            with np.errstate(all="ignore"):
                want = ref[nm].astype(np.float32)
            assert np.array_equal(got.reshape(want.shape), want, equal_nan=True), (nm, keepdims)
        if keepdims == 0:
            continue
        if F in (5, 64):  # k = 1 among several candidates, both directions, ties on the integer grid
            blob1, _ = W.reduce_zoo(2, F, k=1)
            ref1 = W.reduce_reference(xi, 1)
            for nm in ("topk_v0", "topk_i0", "topk_v1", "topk_i1"):
                got = _predict(api, tmp_path, blob1, [xi], "#" + nm)[0]
                assert np.array_equal(got, ref1[nm].astype(np.float32)), (nm, "k = 1")
        # summed operators on generic data: the fixed-order f32 sum of E terms is within E 2^-24 of the sum of magnitudes
        for nm, x in (("r_ReduceMean", xg), ("r_ReduceL2", xg), ("r_ReduceLogSum", xp), ("r_ReduceLogSumExp", xg), ("r_ReduceProd", xg)):
            r = W.reduce_reference(x, k)
            got = _predict(api, tmp_path, blob, [x], "#" + nm)[0].astype(np.float64).reshape(rows, 1)
            want = r[nm]
            rel = (F + 4) * U  # E roundings + the operator's own (divide, sqrt, log: <= 2 ulp each)
            if nm == "r_ReduceMean":
                tol = rel * r["mag_sum"] / F
            elif nm == "r_ReduceL2":
                tol = rel * want
            elif nm == "r_ReduceLogSum":
                tol = rel + 4 * U * np.abs(want)  # d log(s) = ds / s, all terms positive
            elif nm == "r_ReduceLogSumExp":
                tol = rel + 4 * U * (np.abs(want) + np.abs(x).max(1, keepdims=True)) + 4 * U  # + exp's 2 ulp per term
            else:
                tol = rel * np.abs(want)  # E - 1 multiplications
                if not np.isfinite(want).all() or (np.abs(want) < 1e-30).any():
                    continue
            assert (np.abs(got - want) <= tol).all(), (nm, np.abs(got - want).max(), tol.min())


def test_reduce_window_and_nan(api, tmp_path):
    rng = np.random.default_rng(5)
    x = rng.integers(-8, 9, (65, 3, 5)).astype(np.float32)
    blob, names = W.reduce_zoo(3, 5, T=3)
    ref = W.reduce_reference(x)
    for nm in names:
        if nm in EXACT or nm[0] == "b":
            got = _predict(api, tmp_path, blob, [x.reshape(65, 15)], "#" + nm)[0]  # (the C ABI takes the window flat)
            with np.errstate(all="ignore"):
                want = ref[nm].astype(np.float32)
            assert np.array_equal(got.reshape(want.shape), want, equal_nan=True), nm
    # a NaN poisons its own vector only
    x2 = x[:, 0, :].copy()
    x2[3, 2] = np.nan
    blob, names = W.reduce_zoo(2, 5)
    for nm in ("r_ReduceSum", "r_ReduceMax", "r_ReduceMin", "r_ReduceLogSumExp", "r_ReduceL2"):
        got = _predict(api, tmp_path, blob, [x2], "#" + nm)[0].reshape(-1)
        assert np.isnan(got[3]) and not np.isnan(np.delete(got, 3)).any(), nm


def test_autoencoder_end_to_end(api, tmp_path):
    F, H = 12, 4
    blob, w = W.autoencoder(F, H)
    x = np.random.default_rng(9).standard_normal((130, F)).astype(np.float32)
    got = _predict(api, tmp_path, blob, [x])[0].reshape(-1).astype(np.float64)
    w = {k: v.astype(np.float64) for k, v in w.items()}
    x64 = x.astype(np.float64)
    h = np.maximum(x64 @ w["W1"] + w["b1"], 0)
    rec = h @ w["W2"] + w["b2"]
    want = ((x64 - rec) ** 2).mean(1)
    # each layer's f32 sum: (K + 2) 2^-24 of its magnitude; the difference is squared (relative error doubles) and averaged
    mh = np.abs(x64) @ np.abs(w["W1"]) + np.abs(w["b1"])
    mrec = mh @ np.abs(w["W2"]) + np.abs(w["b2"])
    e_rec = (F + 2) * U * mh @ np.abs(w["W2"]) + (H + 2) * U * mrec
    tol = ((2 * np.abs(x64 - rec) * e_rec + e_rec ** 2).mean(1) + (F + 4) * U * want) * 2
    assert (np.abs(got - want) <= tol).all(), (np.abs(got - want) / tol).max()


# ---- call paths ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("output", ["indices", "distances"])
def test_bits_independent_of_call_path(api, tmp_path, output):
    F, M, rows, k = 30, 1000, 5000, 10
    spec = W.kmeans_spec(F, M, seed=12)
    x = np.random.default_rng(13).standard_normal((rows, F)).astype(np.float32)
    p = W.write(str(tmp_path / "rep.onnx"), W.knn_search_from_spec(spec, k, output))
    api.load_model("nn_rep", p)
    try:
        ref = api.predict("nn_rep", x)
        assert ref.shape == (rows, k)
        for step in (1, 7, 33, 2049):
            n = rows if step > 7 else 200
            parts = [api.predict("nn_rep", x[i:i + step]) for i in range(0, n, step)]
            got = np.concatenate(parts)  # (the last chunk may run past n)
            assert got.shape[0] >= n and np.array_equal(got, ref[:got.shape[0]]), step
        cols = [np.ascontiguousarray(x[:, j]) for j in range(F)]
        assert np.array_equal(api.predict_columns("nn_rep", cols), ref)
        for n in (5, 1000):  # few rows (one block per slice) and many
            assert np.array_equal(api.predict("nn_rep", x[:n]), ref[:n]), n
    finally:
        api.unload_model("nn_rep")
