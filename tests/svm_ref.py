"""The float64 numpy restatement of the SVM contract that the SVM tests compare hip/svm.hip with, the
project's bar for it (`tol_of`, `check`), and whole-number models on which the kernel's f32 arithmetic is exact, so that its
results can be compared bit for bit (`exact_spec`, `exact_table`, `assert_exact`, and the table of exact cases `CASES`, whose strength
tests/test_svm_ref.py proves on the CPU and which tests/test_svm_forms_gpu.py runs on the GPU)."""
from __future__ import annotations

import numpy as np


# ---- the restatement -----------------------------------------------------------------------------------------------------------

def np_kernel(spec, x):
    S = np.asarray(spec["support_vectors"], dtype=np.float64).reshape(spec["n_sv"], spec["features"])
    g, c0, deg = (float(v) for v in spec["kernel_params"])
    dot = x @ S.T
    k = spec["kernel"]
    if k == "LINEAR":
        return dot
    if k == "POLY":
        return (g * dot + c0) ** int(deg)
    if k == "RBF":
        d2 = ((x[:, None, :] - S[None, :, :]) ** 2).sum(-1) if x.shape[0] * S.shape[0] * S.shape[1] < 2e7 else \
            np.maximum((x * x).sum(1)[:, None] + (S * S).sum(1)[None, :] - 2 * dot, 0)
        return np.exp(-g * d2)
    return np.tanh(g * dot + c0)


def platt(d, A, B):
    f = d * A + B
    e = np.exp(-np.abs(f))  # libsvm's overflow-safe form: exp(-f) / (1 + exp(-f)) for f >= 0, else 1 / (1 + exp(f))
    p = np.where(f >= 0, e / (1 + e), 1 / (1 + e))
    p = np.where(p < 1e-7, 1e-7, p)
    return np.where(p > 1 - 1e-7, 1 - 1e-7, p)


def coupling(r, C):
    """libsvm multiclass_probability for one row: r[i][j] pairwise; returns (p, margin of the stopping tests to eps)"""
    Q = np.zeros((C, C))
    for t in range(C):
        for j in range(C):
            if j != t:
                Q[t, t] += r[j, t] * r[j, t]
                Q[t, j] = -r[j, t] * r[t, j]
    p = np.full(C, 1.0 / C)
    eps, margin = 0.005 / C, np.inf
    for _ in range(max(100, C)):
        Qp = Q @ p
        pQp = p @ Qp
        err = np.abs(Qp - pQp).max()
        margin = min(margin, abs(err - eps) / eps)
        if err < eps:
            break
        for t in range(C):
            diff = (-Qp[t] + pQp) / Q[t, t]
            p[t] += diff
            pQp = (pQp + diff * (diff * Q[t, t] + 2 * Qp[t])) / (1 + diff) / (1 + diff)
            Qp = (Qp + diff * Q[t, :]) / (1 + diff)
            p /= 1 + diff
    return p, margin


def np_svm(spec, x32):
    """dict: d [N, P] decisions (regressor: [N, 1]) with their magnitudes sum_s |coef K|, label, scores as served before post_transform"""
    x = x32.astype(np.float64)
    K = np_kernel(spec, x)
    coef = np.asarray(spec["coefficients"], dtype=np.float64)
    rho = np.asarray(spec["rho"], dtype=np.float64)
    out = {}
    if spec["kind"] != "classifier":
        t = K * coef[0][None, :]
        d = t.sum(1) + rho[0]
        out["d"], out["mag"] = d[:, None], np.abs(t).sum(1)[:, None]
        out["scores"] = np.where(d > 0, 1.0, -1.0)[:, None] if spec["kind"] == "one_class" else d[:, None]
        return out
    C = spec["classes"]
    b = np.concatenate([[0], np.cumsum(spec["vectors_per_class"])])
    ds, mags, pairs = [], [], []
    for i in range(C):
        for j in range(i + 1, C):
            ti = K[:, b[i]:b[i + 1]] * coef[j - 1, b[i]:b[i + 1]]
            tj = K[:, b[j]:b[j + 1]] * coef[i, b[j]:b[j + 1]]
            ds.append(ti.sum(1) + tj.sum(1) + rho[len(pairs)])
            mags.append(np.abs(ti).sum(1) + np.abs(tj).sum(1))
            pairs.append((i, j))
    d, mag = np.stack(ds, 1), np.stack(mags, 1)
    votes = np.zeros((x.shape[0], C), dtype=np.int64)
    for p, (i, j) in enumerate(pairs):
        win = d[:, p] > 0
        votes[:, i] += win
        votes[:, j] += ~win
    out.update(d=d, mag=mag, label=np.asarray(spec["labels"], dtype=np.float64)[np.argmax(votes, 1)])
    if spec.get("prob_a") is None:
        out["scores"] = np.stack([d[:, 0], -d[:, 0]], 1) if C == 2 else d
        return out
    A, B = np.asarray(spec["prob_a"], np.float64), np.asarray(spec["prob_b"], np.float64)
    r = platt(d, A[None, :], B[None, :])
    if C == 2:
        out["scores"] = np.stack([r[:, 0], 1 - r[:, 0]], 1)
        out["coupling_margin"] = np.full(x.shape[0], np.inf)
        return out
    prob = np.full((x.shape[0], C), np.nan)
    margin = np.full(x.shape[0], np.inf)
    for n in range(x.shape[0]):
        if np.isnan(r[n]).any():
            continue
        R = np.zeros((C, C))
        for p, (i, j) in enumerate(pairs):
            R[i, j], R[j, i] = r[n, p], 1 - r[n, p]
        prob[n], margin[n] = coupling(R, C)
    out["scores"], out["coupling_margin"] = prob, margin
    return out


def tol_of(ref):
    return 1e-4 * (np.abs(ref["d"]) + ref["mag"]) + 1e-6


def check(spec, ref, got, what):
    """`what`: 'label', 'scores' (decisions / values / probabilities as served, post_transform NONE)"""
    tol = tol_of(ref)
    if what == "label":
        near = (np.abs(ref["d"]) <= tol).any(1)
        print(f"{int(near.sum())} of {near.size} rows excluded (a decision within the tolerance of 0)")
        assert near.mean() < 0.01
        got = got.reshape(-1)
        assert np.array_equal(got[~near], ref["label"][~near].astype(np.float32))
        return
    want = ref["scores"]
    assert got.shape == want.shape, (got.shape, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    g, w = got.astype(np.float64)[~nan], want[~nan]
    if spec["kind"] == "one_class":
        near = (np.abs(ref["d"][:, 0]) <= tol[:, 0])
        ok = (got[:, 0] == want[:, 0]) | near
        assert ok[~np.isnan(want[:, 0])].all()
        return
    if spec["kind"] != "classifier" or spec.get("prob_a") is None:
        if spec["kind"] == "classifier" and spec["classes"] == 2:
            tol = np.concatenate([tol, tol], 1)
        err = np.abs(g - w)
        bad = err > tol[~nan]
        assert not bad.any(), f"{bad.sum()} / {bad.size} out of tolerance; worst {err.max():.3e}"
        return
    # probabilities: a decision error e moves r_ij by at most |A| e / 4; the coupling keeps that order unless its stopping test
    # falls within that error of eps (those rows are counted and excluded)
    A = np.abs(np.asarray(spec["prob_a"], np.float64))
    etol = (tol * A[None, :] / 4).max(1, keepdims=True) * 10 + 1e-6
    err = np.abs(got.astype(np.float64) - want)
    unstable = ref["coupling_margin"] < 1e-3
    print(f"{int(unstable.sum())} of {unstable.size} rows excluded (coupling stop within 1e-3 of eps)")
    assert unstable.sum() <= max(2, 0.01 * unstable.size)
    bad = (err > etol) & ~unstable[:, None] & ~nan
    assert not bad.any(), f"{bad.sum()} / {bad.size} out of tolerance; worst {np.nanmax(err):.3e}"


def worst_ratio(spec, ref, got):
    """max |got - want| / tol over the decisions or values as served without prob_a / prob_b: the figure `check` bounds by 1 (NaN rows left out)"""
    tol = tol_of(ref)
    if spec["kind"] == "classifier" and spec["classes"] == 2:
        tol = np.concatenate([tol, tol], 1)
    want = ref["scores"]
    ok = ~np.isnan(want)
    return float((np.abs(got.astype(np.float64) - want)[ok] / tol[ok]).max())


def same_bits(got, want64):
    """`got` (f32, as served) against float32(`want64`), bit for bit: the sign of a zero included"""
    want = np.asarray(want64, dtype=np.float64).astype(np.float32)
    return got.shape == want.shape and np.array_equal(np.ascontiguousarray(got).view(np.uint32), want.view(np.uint32))


# ---- whole-number models: exact in f32 ---------------------------------------------------------------------------------------------
# On whole numbers LINEAR and POLY are exact from end to end in hip/svm.hip: stage 1 is a chain of f32 fma on integers, the powers are
# integer products, stage 2 is f32 fma or MFMA on integers, the partials are stored as they are and the reduction is f64.  While every
# value stays below 2^24 any order of summation gives the one right answer, and float32(np_svm(...)) is what the kernel must serve.

LIMIT = float(2 ** 24)


def exact_spec(kernel="LINEAR", features=9, kind="regressor", per_class=None, n_sv=33, degree=3, coef0=0, probabilities=False, labels=None,
               seed=0):
    """A seeded whole-number SVM with the keys of onnx_writer.svm_spec().  Each support vector has a few non-zero small integers: SV s
    holds one at feature F - 1 - s (mod F), and where n_SV < F at every n_SV-th feature below it (up to 16 per SV), so that every feature
    -- the last one first -- is read by some SV whenever n_SV allows; the rest at seeded positions.  Coefficients are non-zero small
    integers, rho small integers; at every other pair rho cancels the decision of an all-zero row, so that d == 0 occurs (exact_table puts
    such a row in).  POLY: gamma = 1, integer coef0, and for degree 16 one non-zero per SV and |x|, |s|, |coef0| <= 1, so |base| <= 2.
    "xmax" is the range of the table that keeps the premise of assert_exact()."""
    assert kernel in ("LINEAR", "POLY") and kind in ("regressor", "one_class", "classifier")
    cls = kind == "classifier"
    per_class = [int(v) for v in per_class] if cls else [int(n_sv)]
    n_sv, C, F = int(sum(per_class)), (len(per_class) if cls else 1), int(features)
    deg, c0 = (int(degree), int(coef0)) if kernel == "POLY" else (1, 0)
    rng = np.random.default_rng([seed, F, n_sv, C, deg])
    nnz = min(F, 16, max(3, -(-F // n_sv)))
    if kernel == "POLY" and deg == 16:
        assert abs(c0) <= 1
        nnz, xmax, smax, cmax = 1, 1, 1, 2
    elif kernel == "POLY":
        xmax, smax, cmax = (1, 1, 3) if nnz > 3 else (2, 2, 3)
    else:
        xmax, smax, cmax = 3, 2, 3
    S = np.zeros((n_sv, F))
    for s in range(n_sv):
        pos = {(F - 1 - s) % F} | {F - 1 - s - m * n_sv for m in range(nnz) if n_sv < F and F - 1 - s - m * n_sv >= 0}
        while len(pos) < nnz:
            pos.add(int(rng.integers(F - 1)))  # (feature F - 1 only where the rule above puts it)
        for k in sorted(pos):
            S[s, k] = int(rng.choice([-1, 1])) * int(rng.integers(1, smax + 1))
    Q, P = (C - 1, C * (C - 1) // 2) if cls else (1, 1)
    coef = rng.choice([-1, 1], (Q, n_sv)) * rng.integers(1, cmax + 1, (Q, n_sv))
    rho = rng.integers(-3, 4, P)
    k0 = c0 ** deg if kernel == "POLY" else 0  # K(0, s) for every s
    b = np.concatenate([[0], np.cumsum(per_class)])
    if cls:
        p = 0
        for i in range(C):
            for j in range(i + 1, C):
                if p % 2 == 0:
                    rho[p] = -k0 * (coef[j - 1, b[i]:b[i + 1]].sum() + coef[i, b[j]:b[j + 1]].sum())
                p += 1
    else:
        rho[0] = -k0 * coef.sum()
    f32 = lambda a: np.asarray(a, dtype=np.float32)  # noqa: E731
    return {
        "kind": kind, "features": F, "kernel": kernel, "post": "NONE", "classes": C,
        "labels": list(labels) if labels is not None else list(range(C)),
        "vectors_per_class": per_class, "n_sv": n_sv, "support_vectors": f32(S), "coefficients": f32(coef), "rho": f32(rho),
        "kernel_params": f32([1.0, c0, deg]),
        "prob_a": f32(-rng.uniform(0.05, 0.3, P)) if (cls and probabilities) else None,
        "prob_b": f32(rng.normal(0, 0.2, P)) if (cls and probabilities) else None,
        "xmax": xmax,
    }


def exact_table(spec, rows, seed=0):
    """[rows, F] dense integers in [-xmax, xmax] (f32); with more than one row, the middle row is all zeros (d == 0 at every other pair)"""
    rng = np.random.default_rng([seed, rows, spec["features"]])
    x = rng.integers(-spec["xmax"], spec["xmax"] + 1, (rows, spec["features"])).astype(np.float32)
    if rows > 1:
        x[rows // 2] = 0
    return x


def assert_exact(spec, x):
    """The premise of a bit-for-bit comparison, computed in float64; returns np_svm(spec, x).  Every input is a whole number; every partial
    sum of a dot product, every power the squaring loop forms on the way to the result, every kernel value and, per row and pair,
    sum |coef K| + |rho| -- which bounds every partial sum of stage 2 and of the reduction -- is below 2^24."""
    assert spec["kernel"] in ("LINEAR", "POLY")
    x64 = np.asarray(x, dtype=np.float64)
    S = np.asarray(spec["support_vectors"], dtype=np.float64).reshape(spec["n_sv"], spec["features"])
    coef, rho = np.asarray(spec["coefficients"], dtype=np.float64), np.asarray(spec["rho"], dtype=np.float64)
    g, c0, deg = (float(v) for v in spec["kernel_params"])
    for a in (x64, S, coef, rho, np.asarray([c0, deg])):
        assert np.array_equal(a, np.rint(a)), "not whole numbers"
    assert (np.abs(x64) @ np.abs(S).T).max(initial=0.0) < LIMIT
    if spec["kernel"] == "POLY":
        assert g == 1.0 and 1 <= deg <= 16
        base, r, e = x64 @ S.T + c0, 1.0, int(deg)
        while e:  # the loop of svm.hip's kernel_fn, without its last (unused) squaring
            if e & 1:
                r = r * base
                assert np.abs(r).max(initial=0.0) < LIMIT
            e >>= 1
            if e:
                base = base * base
                assert np.abs(base).max(initial=0.0) < LIMIT
    ref = np_svm(spec, x)
    assert (ref["mag"] + np.abs(rho)[None, :]).max() < LIMIT
    return ref


def served(spec, ref):
    """the arrays a caller can be served from this model: scores (values, one-class signs, decisions or probabilities) and label"""
    return [ref["scores"]] + ([ref["label"]] if spec["kind"] == "classifier" else [])


def mutations(spec):
    """name -> a copy of `spec` with one subtle error, for each error the model's shape allows: the last support vector dropped; two
    different support vectors' different coefficients exchanged inside one 32-SV tile (needs a tile with two such SVs); feature F - 1 of
    the support vectors zeroed; two classes' coefficient rows exchanged -- the block(i, j - 1) + block(j, i) pairing (needs C >= 3)."""
    n, F = spec["n_sv"], spec["features"]
    S = np.asarray(spec["support_vectors"], dtype=np.float32).reshape(n, F)
    coef = np.asarray(spec["coefficients"], dtype=np.float32)
    out = {}
    vpc = list(spec["vectors_per_class"])
    last = max(c for c in range(len(vpc)) if vpc[c] > 0)
    vpc[last] -= 1
    out["last_sv_dropped"] = dict(spec, n_sv=n - 1, vectors_per_class=vpc, support_vectors=S[:-1].copy(), coefficients=coef[:, :-1].copy())
    b = np.concatenate([[0], np.cumsum(spec["vectors_per_class"])])
    for c in range(len(b) - 1):
        pair = next(((b[c] + m, b[c] + m + 1) for m in range(int(b[c + 1] - b[c]) - 1)
                     if m // 32 == (m + 1) // 32 and not np.array_equal(coef[:, b[c] + m], coef[:, b[c] + m + 1])
                     and not np.array_equal(S[b[c] + m], S[b[c] + m + 1])), None)
        if pair:
            sw = coef.copy()
            sw[:, list(pair)] = sw[:, list(pair[::-1])]
            out["coefficients_exchanged_in_a_tile"] = dict(spec, coefficients=sw)
            break
    z = S.copy()
    z[:, F - 1] = 0
    out["last_feature_zeroed"] = dict(spec, support_vectors=z)
    if coef.shape[0] >= 2:
        sw = coef.copy()
        sw[[0, 1]] = sw[[1, 0]]
        out["class_rows_exchanged"] = dict(spec, coefficients=sw)
    return out


# ---- the exact cases ---------------------------------------------------------------------------------------------------------------
# A workgroup of svm_kernel_kernel has as many waves (4, 2, 1) as keep its row tiles, 32 nw (F_pad + 4) floats, within 64 KB of LDS; a
# single wave's tile above 64 KB takes opt-in dynamic LDS.  From kernel_launch: 4 waves up to F = 120, 2 up to 248, 1 up to 504, opt-in
# from 505 to the load cap 1024.

FORM_F = (1, 7, 8, 9, 120, 121, 248, 249, 504, 505, 561, 1024)
STAGE2_C = (2, 3, 4, 5, 6, 9, 10, 33, 34, 64)
DEGREES = (1, 2, 3, 16)


def launch_form(F):
    """(waves per workgroup, LDS bytes, opt-in): the arithmetic of kernel_launch in hip/svm.hip"""
    F_pad, nw = (F + 7) // 8 * 8, 4
    while nw > 1 and nw * 32 * (F_pad + 4) * 4 > 64 * 1024:
        nw //= 2
    lds = nw * 32 * (F_pad + 4) * 4
    return nw, lds, lds > 64 * 1024


def form_rows(F):
    nw = launch_form(F)[0]
    return [1, 32 * nw - 1, 32 * nw, 32 * nw + 1]


def stage2_width(spec):
    """QW of host/svm.cpp: 1, 2, 4, 8 on the VALU, 32 or 64 on the second MFMA"""
    Q = spec["classes"] - 1 if spec["kind"] == "classifier" else 1
    return next(w for w in (1, 2, 4, 8, 32, 64) if Q <= w)


# seeds moved on where tests/test_svm_ref.py found the first draw too weak (two support vectors' shares of feature F - 1 cancelling, ...)
RESEED = {"LINEAR-F7-binary": 1, "LINEAR-F8-regressor97": 1, "LINEAR-F1-one_class": 12, "POLY-F1-one_class": 2}


def _cases():
    out = []
    for kernel in ("LINEAR", "POLY"):
        for n, F in enumerate(FORM_F):
            poly = dict(degree=(2, 3)[n % 2], coef0=(-1, 1, -2, 2)[n % 4])
            models = [(f"regressor{m}", dict(kind="regressor", n_sv=m)) for m in (1, 32, 33, 97)]
            models += [("one_class", dict(kind="one_class", n_sv=33)), ("binary", dict(kind="classifier", per_class=[32, 33], labels=[4, 9])),
                       ("three", dict(kind="classifier", per_class=[32, 0, 37], labels=[7, 5, 2]))]
            for tag, kw in models:
                # (one-class serves a sign only: a longer table as well, or no row may sit close enough to 0 to show a subtle error)
                name = f"{kernel}-F{F}-{tag}"
                out.append(dict(name=name, group="forms", key=(kernel, F), rows=form_rows(F) + ([1000] if tag == "one_class" else []),
                                kw=dict(kernel=kernel, features=F, seed=n + 100 * RESEED.get(name, 0), **poly, **kw)))
        for n, C in enumerate(STAGE2_C):
            per_class = ([33, 1, 32] + [int(v) for v in np.random.default_rng(C).integers(1, 34, C)])[:C] if C > 2 else [33, 32]
            out.append(dict(name=f"{kernel}-C{C}", group="stage2", key=(kernel, C), rows=[1, 129],
                            kw=dict(kernel=kernel, features=9, kind="classifier", per_class=per_class, labels=list(range(100, 100 + C)),
                                    degree=(3, 2)[n % 2], coef0=(-1, 2)[n % 2], seed=C)))
    for deg in DEGREES:
        for tag, kw in (("regressor", dict(kind="regressor", n_sv=33)), ("three", dict(kind="classifier", per_class=[5, 32, 3]))):
            out.append(dict(name=f"POLY-degree{deg}-{tag}", group="degrees", key=deg, rows=[129],
                            kw=dict(kernel="POLY", features=9, degree=deg, coef0=-1, seed=deg, **kw)))
    per_class = [int(v) for v in np.random.default_rng(16).integers(1, 6, 16)]
    out.append(dict(name="LINEAR-C16-probabilities", group="prob16", key=16, rows=[65],
                    kw=dict(kernel="LINEAR", features=9, kind="classifier", per_class=per_class, probabilities=True, seed=16)))
    return out


CASES = _cases()
BY_NAME = {c["name"]: c for c in CASES}


def cases_of(group, key=None):
    return [c for c in CASES if c["group"] == group and (key is None or c["key"] == key)]


def build(case):
    """(spec, {rows: table}) of an exact case"""
    spec = exact_spec(**case["kw"])
    return spec, {n: exact_table(spec, n, seed=len(case["name"])) for n in case["rows"]}
