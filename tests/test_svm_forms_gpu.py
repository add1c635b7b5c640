"""The SVM kernel (hip/svm.hip) on every launch form and every stage-2 form, exactly and at the value edges, through the C ABI.

LINEAR and POLY run on the whole-number models of tests/svm_ref.py, where the kernel's f32 arithmetic is exact (assert_exact() states and
checks the premise in float64; tests/test_svm_ref.py proves on the CPU that each case sees a dropped support vector, two exchanged
coefficients, an unread feature and two exchanged class rows): decisions, values and [d, -d] equal float32(reference) bit for bit, labels
and one-class signs on every row, d == 0 included.  RBF and SIGMOID run the same forms on small models (n_SV <= 65: one wrong support
vector is far outside the tolerance) at the project's bar, tests/svm_ref.py check() / tol_of(); each test prints its worst err / tol.

Launch forms (kernel_launch: as many waves per workgroup as keep 32 nw (F_pad + 4) floats within 64 KB; above that, one wave with
opt-in dynamic LDS), by F:
    4 waves          F <= 120       F = 1, 7, 8, 9, 120     test_launch_forms_bit_for_bit, test_rbf_sigmoid_wave_forms (F = 9)
    2 waves          121 ... 248    F = 121, 248            test_launch_forms_bit_for_bit, test_rbf_sigmoid_wave_forms (F = 121)
    1 wave           249 ... 504    F = 249, 504            test_launch_forms_bit_for_bit, test_rbf_sigmoid_wave_forms (F = 249)
    1 wave, opt-in   505 ... 1024   F = 505, 561, 1024      test_launch_forms_bit_for_bit, test_rbf_sigmoid_wave_forms (F = 561, 1024)
each at 1, 32 nw - 1, 32 nw and 32 nw + 1 rows (RBF / SIGMOID: the last three).

The 24 instances svm_kernel_kernel<kernel type, QW> (QW from Q = C - 1, or 1 for a regressor: host/svm.cpp):
    QW   Q        LINEAR, POLY                                                              RBF, SIGMOID
    1    1        test_launch_forms_bit_for_bit (regressors, one-class, binary), C = 2 of    test_rbf_sigmoid_wave_forms (regressor),
                  test_stage2_forms_bit_for_bit                                             test_rbf_sigmoid_stage2_forms C = 2
    2    2        test_launch_forms_bit_for_bit (three classes), C = 3                       test_rbf_sigmoid_wave_forms (three classes), C = 3
    4    3, 4     test_stage2_forms_bit_for_bit C = 4, 5                                     test_rbf_sigmoid_stage2_forms C = 5
    8    5 ... 8  test_stage2_forms_bit_for_bit C = 6, 9                                     test_rbf_sigmoid_stage2_forms C = 9
    32   9 ... 32 test_stage2_forms_bit_for_bit C = 10, 33                                   test_rbf_sigmoid_stage2_forms C = 12
    64   33 ... 63 test_stage2_forms_bit_for_bit C = 34, 64                                  test_rbf_sigmoid_stage2_forms C = 40
(POLY additionally at degrees 1, 2, 3 and 16 in test_poly_degrees; C = 16 with probabilities in test_probabilities_at_the_class_cap.)

Worst err / tol, measured on an MI355X (2026-10-21); every test passed, the file in 3.3 s:
  test_rbf_sigmoid_wave_forms, regressor / three classes, worst over the three row counts:
    RBF      F = 9: 0.0005 / 0.0004   121: 0.0004 / 0.0005   249: 0.0003 / 0.0004   561: 0.0004 / 0.0004   1024: 0.0003 / 0.0006
    SIGMOID  F = 9: 0.0005 / 0.0004   121: 0.0004 / 0.0005   249: 0.0003 / 0.0003   561: 0.0002 / 0.0004   1024: 0.0002 / 0.0004
  test_rbf_sigmoid_stage2_forms, C = 2, 3, 5, 9, 12, 40:
    RBF      0.0003  0.0005  0.0006  0.0008  0.0011  0.0019
    SIGMOID  0.0003  0.0005  0.0006  0.0007  0.0010  0.0013
  RBF rows equal to support vectors at offset 1000: 0.0007 (regressor), 0.0010 (three classes); SIGMOID saturated: 0.0036, 0.0029;
  POLY on generic data, degrees 1, 2, 3, 16: regressor 0.0004, 0.0004, 0.0005, 0.0006; three classes 0.0004, 0.0005, 0.0005, 0.0028.
Without the non-finite rule in the row staging (the kernel as it was), test_non_finite_rows fails for SIGMOID with class blocks of 32:
the +-Inf rows are served finite sums of tanh(+-Inf) = +-1; every other case of that test passes either way."""
from __future__ import annotations

from contextlib import contextmanager

import numpy as np
import pytest

from infera_amd import onnx_writer as W
from tests import svm_ref as R
from tests.test_svm_gpu import _sv_like, _table

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api(built):
    from infera_amd import capi

    assert capi.device_count() >= 1, capi.get_devices()
    return capi


@contextmanager
def serve(api, tmp_path, spec, select="", name="svm_forms"):
    """the model of `spec` loaded; yields predict, with the plan's SvmKernel step as predict.step"""
    p = W.write(str(tmp_path / f"{name}.onnx"), W.svm_from_spec(spec, output="label"))
    api.load_model(name, p + select)
    try:
        def predict(x):
            return api.predict(name, x)

        predict.step = next(s for s in api.get_plan(name)["plan"]["steps"] if s["kind"] == "SvmKernel")
        yield predict
    finally:
        api.unload_model(name)


def votes_label(spec, dec):
    """labels by the votes of served decisions [N, P]"""
    C, n = spec["classes"], dec.shape[0]
    votes, p = np.zeros((n, C), dtype=np.int64), 0
    for i in range(C):
        for j in range(i + 1, C):
            votes[np.arange(n), np.where(dec[:, p] > 0, i, j)] += 1
            p += 1
    return np.asarray(spec["labels"], dtype=np.float32)[np.argmax(votes, 1)]


def exact_run(api, tmp_path, case, slices=None):
    """an exact case of tests/svm_ref.py, every table of it: the premise, then bits"""
    spec, tables = R.build(case)
    refs = {n: R.assert_exact(spec, x) for n, x in tables.items()}
    cls = spec["kind"] == "classifier"
    with serve(api, tmp_path, spec, "#probabilities" if cls else "") as m:
        if slices is not None:
            assert m.step["slices"] == slices, m.step
        for n, x in tables.items():
            assert R.same_bits(m(x), refs[n]["scores"]), (case["name"], n)  # values, one-class signs, decisions, [d, -d]
    if cls:
        with serve(api, tmp_path, spec) as m:
            for n, x in tables.items():
                assert np.array_equal(m(x).reshape(-1), refs[n]["label"].astype(np.float32)), (case["name"], n)
    return spec, tables, refs


# ---- 1. every launch form, bit for bit ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("F", R.FORM_F)
@pytest.mark.parametrize("kernel", ["LINEAR", "POLY"])
def test_launch_forms_bit_for_bit(api, tmp_path, kernel, F):
    """F = 1 ... 120: 4 waves; 121 ... 248: 2 waves; 249 ... 504: 1 wave; 505 ... 1024: 1 wave with opt-in LDS (66048 ... 131584 bytes).
    Regressors of 1, 32, 33 and 97 support vectors (97: four tiles, two slices), a one-class model, a binary classifier ([d, -d]) and three
    classes of 32 (no padding), 0 and 37 support vectors, each at 1, 32 nw - 1, 32 nw and 32 nw + 1 rows."""
    nw = R.launch_form(F)[0]
    cases = R.cases_of("forms", (kernel, F))
    assert len(cases) == 7
    for case in cases:
        assert case["rows"][:4] == [1, 32 * nw - 1, 32 * nw, 32 * nw + 1]
        exact_run(api, tmp_path, case, slices={"regressor97": 2, "binary": 2, "three": 2}.get(case["name"].rsplit("-", 1)[1], 1))


# ---- 2. every stage-2 form, bit for bit --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", R.STAGE2_C)
@pytest.mark.parametrize("kernel", ["LINEAR", "POLY"])
def test_stage2_forms_bit_for_bit(api, tmp_path, kernel, C):
    """Q = C - 1 on both sides of every bucket edge (QW 1 | 2 | 4 | 8 on the VALU, 32 | 64 on the second MFMA) and at the class cap 64,
    class blocks of 1 ... 33 support vectors"""
    (case,) = R.cases_of("stage2", (kernel, C))
    spec, tables, refs = exact_run(api, tmp_path, case)
    assert min(spec["vectors_per_class"]) >= 1 and max(spec["vectors_per_class"]) == 33
    n = max(tables)
    if C > 2:  # the reference's label is the label by the votes of its decisions
        assert np.array_equal(votes_label(spec, refs[n]["d"]), refs[n]["label"].astype(np.float32))


# ---- 3. RBF and SIGMOID on the same forms, at the project's bar ------------------------------------------------------------------------

def bar_run(api, tmp_path, spec, xs, tag):
    """check() on the scores of every table in xs (and the label on the longest); returns the worst err / tol"""
    worst = 0.0
    cls = spec["kind"] == "classifier"
    refs = [R.np_svm(spec, x) for x in xs]
    with serve(api, tmp_path, spec, "#probabilities" if cls else "") as m:
        for x, ref in zip(xs, refs):
            got = m(x)
            worst = max(worst, R.worst_ratio(spec, ref, got))
            R.check(spec, ref, got, "scores")
    if cls:
        with serve(api, tmp_path, spec) as m:
            R.check(spec, refs[-1], m(xs[-1]), "label")
    print(f"\n{tag}: worst err / tol = {worst:.4f}")
    return worst


WAVE_F = (9, 121, 249, 561, 1024)  # 4 waves, 2 waves, 1 wave, 1 wave with opt-in LDS, the same at the load cap


@pytest.mark.parametrize("F", WAVE_F)
@pytest.mark.parametrize("kernel", ["RBF", "SIGMOID"])
def test_rbf_sigmoid_wave_forms(api, tmp_path, kernel, F):
    rows = R.form_rows(F)[1:]
    x = _table(rows[-1], F, seed=F)
    for kind, C in (("regressor", 1), ("classifier", 3)):
        spec = _sv_like(W.svm_spec(features=F, n_sv=65, kind=kind, classes=C, kernel=kernel, seed=F + C), x)
        bar_run(api, tmp_path, spec, [x[:n] for n in rows], f"{kernel} F = {F} ({R.launch_form(F)[0]} waves) {kind}")


@pytest.mark.parametrize("C", [2, 3, 5, 9, 12, 40])
@pytest.mark.parametrize("kernel", ["RBF", "SIGMOID"])
def test_rbf_sigmoid_stage2_forms(api, tmp_path, kernel, C):
    """one C per stage-2 width: QW = 1, 2, 4, 8 (VALU), 32, 64 (MFMA)"""
    F = 9
    x = _table(129, F, seed=C)
    spec = _sv_like(W.svm_spec(features=F, n_sv=65, classes=C, kernel=kernel, seed=40 + C), x)
    assert R.stage2_width(spec) == {2: 1, 3: 2, 5: 4, 9: 8, 12: 32, 40: 64}[C]
    ref = R.np_svm(spec, x)
    with serve(api, tmp_path, spec, "#probabilities") as m:
        dec = m(x)
    R.check(spec, ref, dec, "scores")
    print(f"\n{kernel} C = {C} (QW {R.stage2_width(spec)}): worst err / tol = {R.worst_ratio(spec, ref, dec):.4f}")
    with serve(api, tmp_path, spec) as m:  # the label follows the votes of the served decisions, on every row
        assert np.array_equal(m(x).reshape(-1), votes_label(spec, dec[:, :1] if C == 2 else dec))


def test_rbf_rows_equal_to_support_vectors_at_offset_1000(api, tmp_path):
    """|x - s|^2 = 0 computed as |x|^2 + |s|^2 - 2 x.s around the center: a rounding below 0 is clamped, K = 1"""
    F = 20
    for kind, C in (("regressor", 1), ("classifier", 3)):
        spec = W.svm_spec(features=F, n_sv=65, kind=kind, classes=C, kernel="RBF", offset=1000.0, gamma=0.05, seed=14 + C)
        x = np.concatenate([np.asarray(spec["support_vectors"], dtype=np.float32).reshape(65, F), _table(64, F, seed=13, offset=1000.0)])
        assert np.abs(R.np_svm(spec, x)["d"]).max() > 0.1
        bar_run(api, tmp_path, spec, [x], f"RBF rows = support vectors, offset 1000, {kind}")


def test_rbf_rows_far_from_every_support_vector(api, tmp_path):
    """rows at 1e15: every K is exactly 0, so d is rho bit for bit, whatever the coefficients"""
    F = 9
    x = np.full((33, F), 1e15, dtype=np.float32)
    near = _table(65, F, seed=3)
    for kind, C in (("regressor", 1), ("one_class", 1), ("classifier", 2), ("classifier", 3)):
        spec = _sv_like(W.svm_spec(features=F, n_sv=65, kind=kind, classes=C, kernel="RBF", seed=50 + C), near)
        rho = np.asarray(spec["rho"], dtype=np.float32)
        assert np.all(rho != 0)
        with serve(api, tmp_path, spec, "#probabilities" if C > 1 else "") as m:
            got = m(x)
        want = np.where(rho > 0, 1, -1) if kind == "one_class" else np.stack([rho[0], -rho[0]]) if C == 2 else rho
        assert R.same_bits(got, np.broadcast_to(want.astype(np.float64), (33, want.size))), kind
        assert R.same_bits(got, R.np_svm(spec, x)["scores"])
        if C > 1:
            with serve(api, tmp_path, spec) as m:
                assert np.array_equal(m(x).reshape(-1), votes_label(spec, np.broadcast_to(rho, (33, rho.size))))


def test_sigmoid_saturated(api, tmp_path):
    """|gamma x.s + coef0| > 20 on most pairs: tanh is +-1 there"""
    F = 9
    x = _table(129, F, seed=61) * np.float32(8)
    for kind, C in (("regressor", 1), ("classifier", 3)):
        spec = _sv_like(W.svm_spec(features=F, n_sv=65, kind=kind, classes=C, kernel="SIGMOID", gamma=1.0, seed=60 + C), x)
        arg = x.astype(np.float64) @ np.asarray(spec["support_vectors"], dtype=np.float64).T + 0.5
        assert (np.abs(arg) > 20).mean() > 0.5 and (arg > 20).any() and (arg < -20).any()
        bar_run(api, tmp_path, spec, [x], f"SIGMOID saturated, {kind}")


# ---- 4. POLY degrees -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("degree", R.DEGREES)
def test_poly_degrees(api, tmp_path, degree):
    """the squaring loop at the bit patterns 1, 10, 11 and 10000: exact models with coef0 = -1 (negative bases under even and odd
    degrees; tests/test_svm_ref.py asserts they occur), then generic data at the bar"""
    cases = R.cases_of("degrees", degree)
    assert len(cases) == 2
    for case in cases:
        spec, _, _ = exact_run(api, tmp_path, case)
        assert int(spec["kernel_params"][2]) == degree and float(spec["kernel_params"][1]) == -1.0
    F = 13
    x = _table(129, F, seed=70 + degree)
    for kind, C in (("regressor", 1), ("classifier", 3)):
        spec = _sv_like(W.svm_spec(features=F, n_sv=65, kind=kind, classes=C, kernel="POLY", degree=degree, gamma=0.05, seed=degree), x)
        bar_run(api, tmp_path, spec, [x], f"POLY degree {degree}, generic data, {kind}")


# ---- 5. probabilities at the cap and at saturation -------------------------------------------------------------------------------------

def test_probabilities_at_the_class_cap(api, tmp_path):
    """C = 16 with prob_a / prob_b (the coupling's 16 x 16 system) on an exact LINEAR model: the decisions entering Platt are exact"""
    (case,) = R.cases_of("prob16")
    spec, tables = R.build(case)
    assert spec["classes"] == 16 and spec["prob_a"] is not None
    for x in tables.values():
        ref = R.assert_exact(spec, x)
        with serve(api, tmp_path, spec, "#probabilities") as m:
            R.check(spec, ref, m(x), "scores")
        with serve(api, tmp_path, spec) as m:
            assert np.array_equal(m(x).reshape(-1), ref["label"].astype(np.float32))
        with serve(api, tmp_path, dict(spec, prob_a=None, prob_b=None), "#probabilities") as m:
            assert R.same_bits(m(x), ref["d"])


@pytest.mark.parametrize("C", [2, 3])
def test_probabilities_saturated(api, tmp_path, C):
    """|A d + B| large on both sides: Platt's sigmoid returns both clamps, 1e-7 and 1 - 1e-7"""
    spec = R.exact_spec(kernel="LINEAR", features=9, kind="classifier", per_class=[5, 6, 4][:C], probabilities=True, seed=80 + C)
    P = C * (C - 1) // 2
    spec["prob_a"], spec["prob_b"] = np.full(P, -3.0, dtype=np.float32), np.full(P, 0.25, dtype=np.float32)
    x = R.exact_table(spec, 129, seed=C)
    ref = R.assert_exact(spec, x)
    r = R.platt(ref["d"], -3.0, 0.25)
    assert (r == 1e-7).any() and (r == 1 - 1e-7).any() and ((r > 1e-7) & (r < 1 - 1e-7)).any()
    if C == 2:
        assert (ref["scores"][:, 0] == 1e-7).any() and (ref["scores"][:, 0] == 1 - 1e-7).any()
    with serve(api, tmp_path, spec, "#probabilities") as m:
        R.check(spec, ref, m(x), "scores")


# ---- 6. non-finite rows ----------------------------------------------------------------------------------------------------------------

BAD = [(2, 0, np.nan), (5, 1, np.nan), (8, 2, np.nan), (11, 0, np.inf), (14, 1, np.inf), (17, 2, np.inf), (20, 0, -np.inf), (23, 1, -np.inf),
       (32, 2, -np.inf)]  # (row, feature: first / middle / last, value); rows 0 ... 31 share a tile, row 32 starts the next


@pytest.mark.parametrize("C", [3, 12], ids=["valu", "mfma"])
@pytest.mark.parametrize("per_class", [32, 33], ids=["no_padding", "padding"])
@pytest.mark.parametrize("kernel", W.SVM_KERNELS)
def test_non_finite_rows(api, tmp_path, kernel, per_class, C):
    """a row with a NaN or +-Inf feature gets NaN decisions, values and probabilities, label classlabels[C - 1] and
    one-class -1, for every kernel type, with class blocks of 32 (no padding support vector) and of 33 (31 of them) alike; every other
    row keeps the bits it has without the bad rows"""
    F = 9
    clean = _table(33, F, seed=90 + C)
    x = clean.copy()
    for row, k, v in BAD:
        x[row, (0, F // 2, F - 1)[k]] = v
    bad = np.asarray([b[0] for b in BAD])
    good = np.setdiff1d(np.arange(33), bad)
    labels = list(range(10, 10 + C))
    for prob in (False, True):
        spec = _sv_like(W.svm_spec(features=F, n_sv=per_class * C, classes=C, per_class=[per_class] * C, kernel=kernel, probabilities=prob,
                                   gamma=0.2 if kernel != "RBF" else None, labels=labels, seed=91), clean)
        with serve(api, tmp_path, spec, "#probabilities") as m:
            got, base = m(x), m(clean)
        assert not np.isnan(base).any()
        assert np.isnan(got[bad]).all(), (prob, got[bad])
        assert np.array_equal(got[good].view(np.uint32), base[good].view(np.uint32)), "a bad row leaked"
        with serve(api, tmp_path, spec) as m:
            got, base = m(x).reshape(-1), m(clean).reshape(-1)
        assert (got[bad] == labels[-1]).all() and np.array_equal(got[good], base[good])
        assert len(set(base.tolist())) > 1
    for kind in ("regressor", "one_class"):
        spec = _sv_like(W.svm_spec(features=F, n_sv=per_class, kind=kind, kernel=kernel, gamma=0.2 if kernel != "RBF" else None, seed=92), clean)
        with serve(api, tmp_path, spec) as m:
            got, base = m(x), m(clean)
        assert np.array_equal(got[good].view(np.uint32), base[good].view(np.uint32)), "a bad row leaked"
        if kind == "regressor":
            assert np.isnan(got[bad]).all() and not np.isnan(base).any()
        else:
            assert (got[bad] == -1).all() and set(base.reshape(-1).tolist()) <= {1.0, -1.0}
