"""tests/svm_ref.py on the CPU (no GPU): the float64 restatement against a naive loop written from INTEGRATION.md section 2.6, and the
exact cases tests/test_svm_forms_gpu.py serves -- each keeps the premise of a bit-for-bit comparison, and each can see a subtle error:
a dropped support vector, two coefficients exchanged inside a tile, a feature that is not read, two classes' coefficient rows exchanged."""
from __future__ import annotations

import math

import numpy as np
import pytest

from infera_amd import onnx_writer as W
from infera_amd import synth
from tests import svm_ref as R


def naive(spec, x):
    """decisions and label, row by row and pair by pair, from the text of INTEGRATION.md 2.6"""
    F, n = spec["features"], spec["n_sv"]
    S = [[float(v) for v in row] for row in np.asarray(spec["support_vectors"], dtype=np.float32).reshape(n, F)]
    coef = [[float(v) for v in row] for row in np.asarray(spec["coefficients"], dtype=np.float32)]
    rho = [float(v) for v in spec["rho"]]
    g, c0, deg = (float(v) for v in spec["kernel_params"])
    first = [sum(spec["vectors_per_class"][:c]) for c in range(spec["classes"] + 1)]
    ds, labels = [], []
    for row in x:
        xr = [float(v) for v in row]
        K = []
        for s in S:
            dot = math.fsum(a * b for a, b in zip(xr, s))
            if spec["kernel"] == "LINEAR":
                K.append(dot)
            elif spec["kernel"] == "POLY":
                K.append((g * dot + c0) ** int(deg))
            elif spec["kernel"] == "RBF":
                K.append(math.exp(-g * math.fsum((a - b) ** 2 for a, b in zip(xr, s))))
            else:
                K.append(math.tanh(g * dot + c0))
        C, d, votes, p = spec["classes"], [], [0] * spec["classes"], 0
        for i in range(C):
            for j in range(i + 1, C):
                v = math.fsum(coef[j - 1][s] * K[s] for s in range(first[i], first[i + 1])) + \
                    math.fsum(coef[i][s] * K[s] for s in range(first[j], first[j + 1])) + rho[p]
                votes[i if v > 0 else j] += 1
                d.append(v)
                p += 1
        ds.append(d)
        labels.append(spec["labels"][votes.index(max(votes))])  # the first maximum
    return np.asarray(ds), np.asarray(labels, dtype=np.float64)


@pytest.mark.parametrize("kernel", W.SVM_KERNELS)
def test_restatement_against_a_naive_loop(kernel):
    F = 7
    x = synth.table(3, 0, 60, F).astype(np.float32)
    spec = W.svm_spec(features=F, n_sv=23, classes=4, per_class=[6, 0, 12, 5], kernel=kernel, degree=3, gamma=0.2, labels=[8, 3, 5, 1], seed=4)
    spec["support_vectors"] = x[::2][:23].copy()
    ref = R.np_svm(spec, x)
    d, label = naive(spec, x)
    assert np.allclose(ref["d"], d, rtol=1e-12, atol=1e-13)
    assert np.abs(d).min() > 1e-9  # no decision close enough to 0 for the two to vote differently
    assert np.array_equal(ref["label"], label)
    assert len(set(label)) > 1


def test_launch_forms_and_stage2_widths_are_all_reached():
    """the boundaries of kernel_launch in hip/svm.hip, and the twelve (LINEAR | POLY, QW) instances among the exact cases"""
    assert [R.launch_form(F)[0] for F in (1, 120, 121, 248, 249, 504, 505, 1024)] == [4, 4, 2, 2, 1, 1, 1, 1]
    assert [R.launch_form(F)[2] for F in (248, 249, 504, 505, 561, 1024)] == [False, False, False, True, True, True]
    assert R.launch_form(504)[1] == 65024 and R.launch_form(505)[1] == 66048 and R.launch_form(1024)[1] == 131584 <= 160 * 1024
    seen = {(c["kw"]["kernel"], R.stage2_width(R.exact_spec(**c["kw"]))) for c in R.CASES}
    assert seen == {(k, w) for k in ("LINEAR", "POLY") for w in (1, 2, 4, 8, 32, 64)}
    assert {R.exact_spec(**c["kw"])["classes"] - 1 for c in R.cases_of("stage2")} >= {4, 5, 8, 9, 32, 33, 63}  # both sides of every bucket


@pytest.mark.parametrize("name", [c["name"] for c in R.CASES])
def test_exact_case_is_exact_and_sees_a_subtle_error(name):
    case = R.BY_NAME[name]
    spec, tables = R.build(case)
    F, n = spec["features"], spec["n_sv"]
    S = np.asarray(spec["support_vectors"]).reshape(n, F)
    if n >= F or -(-F // n) <= 16:
        assert (S != 0).any(0).all(), "a feature no support vector reads"
    assert (S[:, F - 1] != 0).any()
    refs = {rows: R.assert_exact(spec, x) for rows, x in tables.items()}
    rows = max(tables)
    x, ref = tables[rows], refs[rows]
    if rows > 1:
        assert (ref["d"] == 0).any(), "no row with a decision of exactly 0"
    if case["group"] == "degrees":
        g, c0, _ = (float(v) for v in spec["kernel_params"])
        assert ((x.astype(np.float64) @ S.T.astype(np.float64)) * g + c0 < 0).any(), "no negative base"
    muts = R.mutations(spec)
    want = {"last_sv_dropped", "last_feature_zeroed"} | ({"coefficients_exchanged_in_a_tile"} if n > 1 else set()) | \
        ({"class_rows_exchanged"} if spec["classes"] >= 3 else set())
    assert set(muts) == want
    for what, m in muts.items():
        other = R.np_svm(m, x)
        assert any(not np.array_equal(a, b) for a, b in zip(R.served(spec, ref), R.served(m, other))), f"{what} changes nothing served"


def test_tied_votes_occur():
    """the first-maximum rule is pinned only where two classes tie for the most votes"""
    tied = 0
    for case in R.cases_of("forms") + R.cases_of("stage2"):
        spec, tables = R.build(case)
        if spec["classes"] < 3:
            continue
        d = R.np_svm(spec, tables[max(tables)])["d"]
        votes, p, C = np.zeros((d.shape[0], spec["classes"]), dtype=np.int64), 0, spec["classes"]
        for i in range(C):
            for j in range(i + 1, C):
                votes[np.arange(d.shape[0]), np.where(d[:, p] > 0, i, j)] += 1
                p += 1
        tied += int(((votes == votes.max(1, keepdims=True)).sum(1) > 1).sum())
    assert tied > 100, tied


def test_probability_case_stays_inside_the_caps_of_check():
    spec, tables = R.build(R.cases_of("prob16")[0])
    x = tables[max(tables)]
    ref = R.assert_exact(spec, x)
    assert spec["classes"] == 16 and ref["scores"].shape == (x.shape[0], 16)
    assert np.allclose(ref["scores"].sum(1), 1.0, atol=1e-6)
    assert (ref["coupling_margin"] < 1e-3).sum() <= 2
