"""tests/recurrent_ref.py without a GPU: the float64 definition against torch.nn in float64, the fairness of every bar case of
tests/test_recurrent_range_gpu.py (the float32 restatement within a quarter of the bar, from the two references alone), the exactness of
every grid case, evidence that the grid reference notices a swapped column of R or k-group of W, and the identities saturated gates obey."""
from __future__ import annotations

import numpy as np
import pytest

from infera_amd import onnx_writer as W
from tests import recurrent_ref as R


def test_float64_definition_agrees_with_torch():
    torch = pytest.importorskip("torch")
    for op, relu in [("LSTM", False), ("GRU", False), ("RNN", False), ("RNN", True)]:
        for T, F, H, layers, D in [(9, 5, 12, 1, 1), (7, 3, 5, 2, 2), (1, 4, 16, 1, 2)]:
            torch.manual_seed(5)
            kw = dict(input_size=F, hidden_size=H, num_layers=layers, bidirectional=D == 2, batch_first=True)
            m = torch.nn.RNN(nonlinearity="relu" if relu else "tanh", **kw) if op == "RNN" else getattr(torch.nn, op)(**kw)
            spec = W.torch_recurrent_spec(m)  # (float32 parameters, which the float64 module below holds exactly)
            x = R.inputs(11, T, F)
            with torch.no_grad():
                y, st = m.double()(torch.from_numpy(x).double())
            hn = st[0] if isinstance(st, tuple) else st
            y_n, h_n, _ = R.recurrent(spec, x)
            assert np.max(np.abs(y.numpy() - y_n)) <= 1e-12, (op, relu, T, F, H, layers, D)
            assert np.max(np.abs(hn[-D:].permute(1, 0, 2).reshape(11, D * H).numpy() - h_n)) <= 1e-12


def test_float32_mode_is_float32_and_close():
    spec = W.recurrent_spec("GRU", T=5, F=3, H=7, linear_before_reset=0, direction="bidirectional", layers=2, initial=0.5)
    x = R.inputs(9, 5, 3)
    r64, r32 = R.recurrent(spec, x), R.recurrent(spec, x, np.float32)
    assert all(a.dtype == np.float64 for a in r64[:2]) and all(a.dtype == np.float32 for a in r32[:2])
    assert 0.0 < R.verdict(r32[0], r64[0]) <= 0.25  # not the same numbers, and well inside the bar


def test_verdict_rule():
    ref = np.array([1.0, np.nan, np.inf, -np.inf, 0.0])
    assert R.verdict(np.array([1.0 + 5e-5, np.nan, np.inf, -np.inf, 5e-7], np.float32), ref) <= 1.0
    assert R.verdict(np.array([1.0 + 2.5e-4, np.nan, np.inf, -np.inf, 0.0], np.float32), ref) > 1.0
    for bad in ([1.0, 0.0, np.inf, -np.inf, 0.0], [1.0, np.nan, 3e38, -np.inf, 0.0], [1.0, np.nan, np.inf, np.inf, 0.0], [np.nan, np.nan, np.inf, -np.inf, 0.0],
                [1.0, np.nan, np.inf, -np.inf, np.inf]):
        assert R.verdict(np.array(bad, np.float32), ref) == np.inf, bad


def test_non_finite_values_follow_ieee():
    """0 . inf and inf - inf are NaN in the reference; an infinite reading alone saturates its step and leaves the row finite"""
    spec = W.recurrent_spec("LSTM", T=3, F=2, H=4)
    x = R.inputs(3, 3, 2)
    x[1, 1, 0] = np.inf
    y = R.recurrent(spec, x)[0]
    assert np.isfinite(y).all()
    zero = R.copy.deepcopy(spec)
    zero["layers"][0]["W"][0, 2, 0] = 0.0  # 0 . inf in unit 2's input gate
    y = R.recurrent(zero, x)[0]
    assert np.isnan(y[1, 1:, :]).any() and np.isfinite(y[[0, 2]]).all() and np.isfinite(y[1, 0]).all()
    x[1, 1, 1] = -np.inf  # inf - inf wherever the two weights have one sign
    assert np.isnan(R.recurrent(spec, x)[0][1, 1:]).any()


# ---- fairness -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(R.BAR_CASES))
def test_bar_cases_are_fair(name):
    r = R.fairness(name)
    print(f"{name}: float32 = {r:.3f}")
    assert r <= 0.25, (name, r)


@pytest.mark.parametrize("name", [c["name"] for c in R.INF_CASES])
def test_planted_infinities_are_fair_and_stay_in_their_rows(name):
    spec, x, r64, _ = R.reference(name, planted=True)
    clean = R.reference(name)[2]
    assert R.fairness(name, planted=True) <= 0.25
    rows = [r for r, _, _, _ in R.INF_AT]
    keep = np.setdiff1d(np.arange(x.shape[0]), rows)
    assert np.array_equal(r64[0][keep], clean[0][keep])
    for (row, t, _, _) in R.INF_AT:  # forward: steps before the planted one are the clean run's, the planted step is not
        assert np.array_equal(r64[0][row, :t], clean[0][row, :t]) and not np.array_equal(r64[0][row, t], clean[0][row, t])
    assert np.isfinite(r64[0]).all()  # one infinite term per pre-activation: no inf - inf, and no weight is 0 (plant_inf asserts it)


# ---- the grid -----------------------------------------------------------------------------------------------------------------------------

GRID_IDS = ["T%d_F%d_H%d_%s_rows%d" % (s + ("_".join(f"{k}{v}" for k, v in kw.items()) or "forward", rows)) for s, kw, rows in R.all_grid_cases()]


@pytest.mark.parametrize("shape,kw,rows", R.all_grid_cases(), ids=GRID_IDS)
def test_grid_cases_are_exact(shape, kw, rows):
    """assert_exact holds (grid_case asserts it), so float32 numpy in its own summation order gives the float64 bits too"""
    spec, x, (y, yh) = R.grid_case(shape, kw, rows)
    assert np.array_equal(y.astype(np.float32).astype(np.float64), y)
    if shape[0] <= 16:
        y32, yh32, _ = R.recurrent(spec, x, np.float32)
        assert np.array_equal(R.bits(y32), R.bits(y)) and np.array_equal(R.bits(yh32), R.bits(yh))
    assert (y > 0).any() and (y[..., :spec["H"]] == 0).any(), "the ReLU is exercised on both sides"


def test_grid_long_case_fits_as_given():
    """T = 4096 with inputs in [-4, 4]: one recurrent term per step, so the state grows at most linearly -- far below 2^24"""
    for d in ("forward", "reverse"):
        _, _, (y, _) = R.grid_case(R.GRID_LONG[0], dict(direction=d), R.GRID_LONG[1])
        assert 0 < np.abs(y).max() < 2 ** 24


@pytest.mark.parametrize("shape", R.GRID_SHAPES + [R.GRID_LONG[0]], ids=lambda s: "x".join(map(str, s)))
def test_grid_reference_notices_a_swap(shape):
    """Two columns of R exchanged, or two k-groups of W: some output element changes on every grid shape, so the bit-for-bit comparison of
    tests/test_recurrent_range_gpu.py would catch the kernel doing the same.  (1, 1, 1) has nothing to exchange: there the sign of W is."""
    spec, x, (y, _) = R.grid_case(shape, {}, 17 if shape == R.GRID_LONG[0] else 33)
    tried = 0
    for what in ("R", "W"):
        s = R.swapped(spec, what)
        if s is None:
            continue
        tried += 1
        assert not np.array_equal(R.recurrent(s, x)[0], y), (shape, what)
    if not tried:
        assert shape == (1, 1, 1)
        s = R.copy.deepcopy(spec)
        s["layers"][0]["W"] *= -1
        assert s["layers"][0]["W"].any() and not np.array_equal(R.recurrent(s, x)[0], y)


def test_grid_spec_is_what_it_says():
    spec = R.grid_relu_rnn(3, 7, 20, D=2, layers=2, seed=1, initial=True)
    for i, L in enumerate(spec["layers"]):
        assert L["W"].shape == (2, 20, 7 if i == 0 else 40) and np.abs(L["W"]).max() == 2 and np.array_equal(L["W"], np.rint(L["W"]))
        for d in range(2):
            nz = np.argwhere(L["R"][d] != 0)
            assert np.array_equal(nz[:, 0], np.arange(20)) and np.array_equal(nz[:, 1], (5 * np.arange(20) + 3) % 20)
            assert set(np.unique(L["R"][d])) == {-1.0, 0.0, 1.0} and not np.array_equal(L["R"][d] != 0, L["R"][d].T != 0)
        assert np.array_equal(L["B"], np.rint(L["B"])) and np.array_equal(L["h0"], np.rint(L["h0"])) and L["h0"].shape == (2, 20)
    x = R.grid_inputs(5, 3, 7)
    assert x.dtype == np.float32 and np.array_equal(x, np.rint(x)) and np.abs(x).max() == 4


# ---- saturated gates ----------------------------------------------------------------------------------------------------------------------

def test_saturating_touches_one_gate():
    spec = W.recurrent_spec("LSTM", T=2, F=3, H=5, direction="bidirectional")
    s = R.saturating(spec, "f", -1)
    d = s["layers"][0]["B"] - spec["layers"][0]["B"]
    assert np.array_equal(d[:, 10:15], np.full((2, 5), -40, np.float32)) and not np.delete(d, np.s_[10:15], axis=1).any()
    assert all(np.array_equal(s["layers"][0][k], spec["layers"][0][k]) for k in ("W", "R"))
    with pytest.raises(AssertionError):
        R.saturating(spec, "c", 1)


@pytest.mark.parametrize("lbr", [1, 0])
def test_gru_update_gate_of_one_keeps_h0(lbr):
    spec = R.saturating(W.recurrent_spec("GRU", T=8, F=6, H=40, linear_before_reset=lbr, initial=0.5), "z", 1)
    y, yh, _ = R.recurrent(spec, R.inputs(33, 8, 6))
    h0 = spec["layers"][0]["h0"][0].astype(np.float64)
    assert all(np.array_equal(y[:, t], np.tile(h0, (33, 1))) for t in range(8)) and np.array_equal(yh, y[:, -1])


def test_lstm_forget_gate_of_zero_leaves_i_g():
    """f = -40: c_t = i (.) g to the last bit wherever |c_{t-1}| sigmoid(-40 + ...) vanishes beside it -- checked as c_t of the saturated spec
    equals c_t recomputed from h_{t-1} alone"""
    spec = R.saturating(W.recurrent_spec("LSTM", T=8, F=6, H=40, initial=0.5), "f", -1)
    x = R.inputs(33, 8, 6)
    L, H = spec["layers"][0], 40
    Wm, Rm, B = (L[k][0].astype(np.float64) for k in ("W", "R", "B"))
    sig = lambda v: 1.0 / (1.0 + np.exp(-v))  # noqa: E731
    for T in range(1, 9):  # the final cell state after T steps, against i (.) g of step T computed from the state before it
        y, _, yc = R.recurrent(dict(spec, T=T), x[:, :T])
        h = y[:, T - 2] if T > 1 else np.tile(L["h0"][0].astype(np.float64), (33, 1))
        pre = x[:, T - 1].astype(np.float64) @ Wm.T + B[:4 * H] + h @ Rm.T + B[4 * H:]
        ig = sig(pre[:, :H]) * np.tanh(pre[:, 3 * H:])
        assert np.max(np.abs(yc - ig)) <= 1e-15, T


def test_lstm_closed_input_and_open_forget_gate_keep_c0():
    spec = R.saturating(R.saturating(W.recurrent_spec("LSTM", T=8, F=6, H=40, initial=0.5), "i", -1), "f", 1)
    _, _, yc = R.recurrent(spec, R.inputs(33, 8, 6))
    assert np.max(np.abs(yc - spec["layers"][0]["c0"][0].astype(np.float64))) <= 1e-15


def test_identity_cases_of_the_gpu_suite():
    """the references the GPU suite compares with ARE the identities: h0 at every step, c0 at the end"""
    for c in R.IDENTITY_CASES:
        spec, x, (y, yh, yc), _ = R.reference(c["name"])
        L = spec["layers"][0]
        if c["op"] == "LSTM":
            assert np.max(np.abs(yc - L["c0"][0].astype(np.float64))) <= 1e-15
        else:
            assert (y == np.tile(L["h0"][0].astype(np.float64), (x.shape[0], c["T"], 1))).all()


def test_growing_cell_state_reaches_T():
    spec, x, (_, _, yc), _ = R.reference(R.GROW_CASE["name"])
    print("c_T between %.1f and %.1f" % (yc.min(), yc.max()))
    assert yc.min() > 0.9 * 512 and yc.max() <= 512
