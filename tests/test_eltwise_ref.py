"""tests/eltwise_ref.py checked without a GPU: its float64 references against each other, and the CPU oracle (oracle/infera_oracle.c)
against them -- every unary operator over the whole float32 range (SWEEP: zeros, subnormals, exact halves, the exp overflow threshold,
the float limits, +-inf, NaN), the comparison-defined operators at NaN, and the row operators on the regimes of softmax_rows /
normalizer_rows at lengths 3, 17 and 300."""
from __future__ import annotations

import numpy as np
import pytest

from infera_amd import onnx_writer as W
from tests import eltwise_ref as E


@pytest.fixture(scope="module")
def O(built):
    from oracle import oracle

    return oracle


def served(O, tmp_path, blob, x):
    return O.Model(W.write(str(tmp_path / "m.onnx"), blob)).predict(x)


# ---- the helper -------------------------------------------------------------------------------------------------------------------

def test_sweep_holds_the_range():
    s = E.SWEEP
    assert s.dtype == np.float32 and np.isnan(s).sum() == 1 and np.isposinf(s).sum() == 1 and np.isneginf(s).sum() == 1
    assert np.array_equal(E.FINITE, s[np.isfinite(s)]) and len(E.FINITE) == len(s) - 3
    assert (np.signbit(s) & (s == 0)).sum() == 1 and (~np.signbit(s) & (s == 0)).sum() == 1
    tiny = np.finfo(np.float32).tiny
    assert ((np.abs(s) < tiny) & (s != 0)).sum() == 5  # +-1e-45, 1e-40 and +-1e-38 (below 2^-126)
    for v in (1e-38, 1e-20, 1e-7, 1e-3, 0.5, 1, 1.5, 2.5, 3, 5, 6, 8, 10, 17, 20, 50, 87, 88.5, 89, 100, 104, 1e4, 1e30, 3e38):
        assert np.float32(v) in s and np.float32(-v) in s, v
    for v in (0.999999, 1.0000001, 3.5):
        assert np.float32(v) in s, v
    assert len(E.OPERATORS) == 22 and {E.UNARY[k][0] for k in E.UNARY} == set(E.OPERATORS) | {"Swish"}
    t = E.sweep_table(301)
    assert t.shape == (301, 7) and all((t == v).any() or np.isnan(v) for v in s) and np.isnan(t).any()


def test_references_agree_with_each_other():
    v = E.SWEEP
    v64 = v.astype(np.float64)
    eq = lambda a, b: np.testing.assert_allclose(a, b, rtol=1e-14, atol=0, equal_nan=True)
    with np.errstate(all="ignore"):
        eq(E.reference("Swish", v), v64 * E.reference("Sigmoid", v))
        eq(E.reference("Sigmoid", v) + E.reference("Sigmoid", -v), np.where(np.isnan(v), np.nan, 1.0))
        np.testing.assert_allclose(E.reference("Softplus", E.FINITE) - E.reference("Softplus", -E.FINITE), E.FINITE.astype(np.float64), rtol=1e-12, atol=1e-15)
        big = v64 >= 40
        eq(E.reference("Softplus", v)[big], v64[big])  # the right answer above the overflow threshold is v
        eq(E.reference("Elu", v)[v64 < 0], np.expm1(v64[v64 < 0]))
        eq(E.reference("Selu", v), np.float64(np.float32(E.SELU_GAMMA)) * np.where(v64 > 0, v64, np.float64(np.float32(E.SELU_ALPHA)) * np.expm1(np.minimum(v64, 0))))
        eq(E.reference("Neg", v), -v64)
        eq(E.reference("Abs", v), np.abs(v64))
        fin = np.isfinite(v)
        hs = E.reference("HardSwish", v)
        eq(hs[fin], (v64 * np.clip(v64 / 6 + 0.5, 0, 1))[fin])
    # Round: ties to even; Floor <= Round <= Ceil
    halves = np.array([0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 3.5], np.float32)
    assert E.reference("Round", halves).tolist() == [0.0, -0.0, 2.0, -2.0, 2.0, -2.0, 4.0]
    f, r, c = (E.reference(k, E.FINITE) for k in ("Floor", "Round", "Ceil"))
    assert (f <= r).all() and (r <= c).all() and (c - f <= 1).all()
    # the NaN table is what the reference returns at NaN
    nan = np.array([np.nan], np.float32)
    for name, (op, _, _) in E.UNARY.items():
        got = E.reference(name, nan)[0]
        want = E.NAN_TABLE.get(op, np.nan)
        assert (np.isnan(got) and np.isnan(want)) or got == want, (name, got, want)


@pytest.mark.parametrize("length", [3, 17, 300])
def test_row_references(length):
    x, names = E.softmax_rows(length)
    assert set(names) == set(E.REGIMES)
    bad = E.poisoned(names)
    p, lp = E.softmax64(x), E.softmax64(x, log=True)
    assert np.isnan(p[bad]).all() and np.isnan(lp[bad]).all() and np.isfinite(p[~bad]).all()
    np.testing.assert_allclose(p[~bad].sum(1), 1.0, rtol=1e-12)
    with np.errstate(all="ignore"):
        np.testing.assert_allclose(np.exp(lp[~bad]), p[~bad], rtol=1e-9, atol=1e-300)
    names = np.array(names)
    assert (p[[n[0] == "d" for n in names]] == 1.0 / length).all()
    f = names == "f"
    assert (p[f][np.isneginf(x[f])] == 0).all() and np.isneginf(lp[f][np.isneginf(x[f])]).all() and (np.isneginf(x[f]).sum(1) < length).all()
    e = names == "e"
    assert (p[e].max(1) >= 1 - 1e-40 * length).all()
    g = names == "g"
    assert np.allclose(p[g][:, 0::2], 1.0 / ((length + 1) // 2)) and (p[g][:, 1::2] == 0).all()
    x, names = E.normalizer_rows(length)
    names = np.array(names)
    assert set(names) == set(E.NORM_REGIMES)
    sq = np.square(x[names != "nan"].astype(np.float32)).sum(1, dtype=np.float32)
    assert ((sq == 0) | ((sq >= np.finfo(np.float32).tiny) & np.isfinite(sq))).all()  # the band the kernel serves: the f32 sum of squares is a normal number
    live = (names != "nan") & (names != "zero")
    for norm, measure in (("L1", lambda y: np.abs(y).sum(1)), ("L2", lambda y: np.sqrt(np.square(y).sum(1))), ("MAX", lambda y: np.abs(y).max(1))):
        y = E.normalizer64(x, norm)
        np.testing.assert_allclose(measure(y[live]), 1.0, rtol=1e-12)
        assert (y[names == "zero"] == 0).all()
        nan_rows = np.isnan(y[names == "nan"])
        assert nan_rows.all() if norm != "MAX" else (nan_rows == np.isnan(x[names == "nan"])).all()


# ---- the oracle -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(E.UNARY))
def test_oracle_unary_over_the_sweep(O, tmp_path, name):
    x = E.sweep_table(301)
    got = served(O, tmp_path, E.unary_graph(name, 7), x)
    ok, ratio = E.verdict(got, x, name)
    print(f"oracle {name}: worst error / bar = {ratio.max():.3f}")
    assert ok.all(), E.describe(ok, x, got, E.reference(name, x))


def test_oracle_matches_the_nan_table(O, tmp_path):
    nan = np.full((3, 7), np.nan, np.float32)
    for name, (op, _, _) in E.UNARY.items():
        if op in E.NAN_TABLE:
            got = served(O, tmp_path, E.unary_graph(name, 7), nan)
            want = E.NAN_TABLE[op]
            assert np.isnan(got).all() if np.isnan(want) else (got == want).all(), (name, got[0], want)
    c = np.array([-2.0, -0.5, 0.0, 0.25, 1.0, 3.0, 100.0], np.float32)
    for op in ("Min", "Max", "PRelu"):
        for left in (False, True) if op != "PRelu" else (False,):
            got = served(O, tmp_path, E.binary_const_graph(op, c, 7, left=left), nan)
            assert np.isnan(got).all() if op == "PRelu" else (got == c).all(), (op, left, got[0])


@pytest.mark.parametrize("length", [3, 17, 300])
@pytest.mark.parametrize("op", ["Softmax", "LogSoftmax", "NormL1", "NormL2", "NormMAX"])
def test_oracle_rows(O, tmp_path, op, length):
    x, names = E.row_batch(op, length)
    model = O.Model(W.write(str(tmp_path / "r.onnx"), E.row_graph(op, length)))
    zeroed = x.copy()
    zeroed[E.poisoned(names)] = 0
    worst = E.check_rows(op, x, names, model.predict(x), model.predict(zeroed))
    print(f"oracle {op} length {length}: worst error / bar = {worst:.3f}")
