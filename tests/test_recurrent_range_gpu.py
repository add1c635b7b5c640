"""rnn_kernel<OP> (hip/rnn.hip) through the C ABI against the float64 definition of tests/recurrent_ref.py, on the code paths
tests/test_recurrent_gpu.py does not reach: hidden-unit tiles dealt unevenly over the waves (9, 13, 17 tiles on 8 waves), the second MFMA
phase of GRU linear_before_reset = 0 with several tiles per wave, the tail loop of the x_t fetch in every input order and direction, dynamic
LDS on either side of the 64 KB opt-in, the column-major chunk beyond one forward LSTM, T = 1, 2, 512 and 4096, saturated gates, a cell
state of hundreds, and infinite readings.

Two kinds of claim.  The ReLU RNN on an integer grid (recurrent_ref.grid_relu_rnn, exactness asserted by assert_exact from the float64
reference alone) is compared BIT FOR BIT: a swapped k-group, a padded unit that is not 0 or a stale h copy cannot hide under a tolerance.
Every other case is a bar claim, |served - float64| <= 1e-4 |ref| + 1e-6 by recurrent_ref.verdict, and obeys the fairness rule case by
case: the float32 restatement is asserted within a quarter of the bar before the kernel is asserted within it.  Every test asserts from
the plan that one Recurrent step per layer of the expected geometry served it.  Each bar case prints its worst error as a share of the
bar and the float32 restatement's (profiles/recurrent_range_ratios.txt holds a run's lines)."""
from __future__ import annotations

import numpy as np
import pytest

from infera_amd import onnx_writer as W
from tests import recurrent_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api(built):
    from infera_amd import capi

    assert capi.device_count() >= 1, capi.get_devices()
    return capi


class Served:
    """one loaded model, checked against its spec: one Recurrent step per layer with the expected T, F, H, D, the last one writing `output`"""

    def __init__(self, api, tmp_path, spec, output="Y", name="recurrent_range", **kw):
        self.api, self.name = api, name
        tail = {"Y": "seq", "Y_h": "y_h", "Y_c": "y_c"}[output]
        api.load_model(name, W.write(str(tmp_path / "m.onnx"), W.recurrent_from_spec(spec, flat=True, tail=tail, **kw)))
        try:
            steps = api.get_plan(name)["plan"]["steps"]
            op, T, F, H, D = spec["op"], spec["T"], spec["F"], spec["H"], spec["D"]
            n = len(spec["layers"])
            assert [s["kind"] for s in steps] == ["Recurrent"] * n, steps
            assert [(s["op"], s["T"], s["F"], s["H"], s["D"]) for s in steps] == [(op, T, F if i == 0 else D * H, H, D) for i in range(n)], steps
            assert [s["output"] for s in steps] == ["Y"] * (n - 1) + [output] and all(s["direction"] == spec["direction"] for s in steps), steps
            if op == "GRU":
                assert all(s["linear_before_reset"] == spec["linear_before_reset"] for s in steps), steps
            if op == "RNN":
                assert all(s["activation"] == spec["activation"] for s in steps), steps
        except BaseException:
            api.unload_model(name)
            raise

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.api.unload_model(self.name)

    def rows(self, x):
        return self.api.predict(self.name, np.ascontiguousarray(x.reshape(x.shape[0], -1), np.float32))

    def columns(self, x):
        """the same table as one contiguous vector per column: the column-major staged chunk"""
        flat = x.reshape(x.shape[0], -1)
        return self.api.predict_columns(self.name, [np.ascontiguousarray(flat[:, j]) for j in range(flat.shape[1])])


def same_bits(got, ref):
    return got.size == np.size(ref) and np.array_equal(R.bits(got).reshape(-1), R.bits(ref).reshape(-1))


# ---- a. exact layout, bit for bit ---------------------------------------------------------------------------------------------------------

def grid_check(api, tmp_path, shape, kw, rows_list, table_rows=33, columns=False, **form):
    spec, x, (y, yh) = R.grid_case(shape, kw, table_rows)
    for output, ref in (("Y", y), ("Y_h", yh)):
        with Served(api, tmp_path, spec, output, **form) as m:
            for n in rows_list:
                got = m.columns(x[:n]) if columns else m.rows(x[:n])
                assert same_bits(got, ref[:n]), (shape, kw, output, n, int((R.bits(got).reshape(-1) != R.bits(ref[:n]).reshape(-1)).sum()))


@pytest.mark.parametrize("shape", R.GRID_SHAPES, ids=lambda s: "T%d_F%d_H%d" % s)
def test_grid_forward(api, tmp_path, shape):
    """rows 1, 16, 17 and 33 of one table: a single row, a full row tile, a second tile with one live row, three tiles"""
    grid_check(api, tmp_path, shape, {}, R.GRID_ROWS)


@pytest.mark.parametrize("form", list(R.GRID_FORMS))
@pytest.mark.parametrize("shape", R.GRID_FORM_SHAPES, ids=lambda s: "T%d_F%d_H%d" % s)
def test_grid_directions_layers_and_initial_state(api, tmp_path, shape, form):
    kw, forms = R.GRID_FORMS[form]
    for f, initial in forms:
        grid_check(api, tmp_path, shape, kw, R.GRID_ROWS, form=f, initial=initial)


@pytest.mark.parametrize("shape,kw,rows", R.GRID_COLUMNS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_grid_through_columns(api, tmp_path, shape, kw, rows):
    """predict_columns stages one column-major chunk [T F][rows]; rows is no multiple of 16, so the last row tile is partly out of range"""
    grid_check(api, tmp_path, shape, kw, [rows], table_rows=rows, columns=True)


@pytest.mark.parametrize("direction", ["forward", "reverse"])
def test_grid_longest_sequence(api, tmp_path, direction):
    """T = 4096, the cap: the grid as given fits (one recurrent term per step grows the state linearly; assert_exact checks it)"""
    shape, rows = R.GRID_LONG
    grid_check(api, tmp_path, shape, dict(direction=direction), [rows], table_rows=rows)


# ---- the bar cases ------------------------------------------------------------------------------------------------------------------------

def report(name, rk, r32):
    print(f"{name}: worst error / bar = {rk:.3f}, float32 = {r32:.3f}")


def bar_check(api, tmp_path, name, planted=False):
    """the fairness rule, then the kernel: Y and every tail the case reads.  Returns the served Y."""
    case = R.BAR_CASES[name]
    spec, x, r64, _ = R.reference(name, planted)
    r32 = R.fairness(name, planted)
    with Served(api, tmp_path, spec) as m:
        got = m.rows(x)
    rk = R.verdict(got, r64[0])
    for tail in case["tails"]:
        output, i = {"y_h": ("Y_h", 1), "y_c": ("Y_c", 2)}[tail]
        with Served(api, tmp_path, spec, output) as m:
            rk = max(rk, R.verdict(m.rows(x), r64[i]))
    report(name + (" planted" if planted else ""), rk, r32)
    assert r32 <= 0.25, (name, r32)
    assert rk <= 1.0, (name, rk)
    return got


def names(cases):
    return [c["name"] for c in cases]


# ---- b. tile distribution -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", names(R.TILE_CASES))
def test_tile_distribution(api, tmp_path, name):
    """1, 8, 9, 13, 17 and 32 tiles of 16 units on up to 8 waves, for every operator; at 9 and 17 tiles also two bidirectional layers with an
    initial state; at 9 tiles the Y_h tail (and Y_c) as well"""
    bar_check(api, tmp_path, name)


@pytest.mark.parametrize("name", R.TILE_COLUMNS)
def test_gru_second_phase_through_columns(api, tmp_path, name):
    """GRU linear_before_reset = 0 with two and three tiles on a wave: the column-major chunk gives the row-major call's bits"""
    spec, x, _, _ = R.reference(name)
    with Served(api, tmp_path, spec) as m:
        assert same_bits(m.columns(x), m.rows(x))


# ---- c. time edges ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", names(R.TIME_CASES))
def test_one_and_two_steps(api, tmp_path, name):
    got = bar_check(api, tmp_path, name)
    if R.BAR_CASES[name]["T"] == 1:  # Y's only step IS the final state, in both directions
        spec, x, _, _ = R.reference(name)
        with Served(api, tmp_path, spec, "Y_h") as m:
            assert same_bits(got, m.rows(x))


@pytest.mark.parametrize("name", names(R.LONG_CASES))
def test_512_steps(api, tmp_path, name):
    bar_check(api, tmp_path, name)


# ---- d. value edges -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", names(R.SAT_CASES))
def test_saturated_gates(api, tmp_path, name):
    bar_check(api, tmp_path, name)


@pytest.mark.parametrize("name", names(R.IDENTITY_CASES))
def test_saturated_identities(api, tmp_path, name):
    """z = 1: the reference IS h0 at every step; i = 0 and f = 1: the final cell state IS c0 (tests/test_recurrent_ref.py asserts both of
    the reference); the kernel within the bar of it"""
    bar_check(api, tmp_path, name)


def test_cell_state_of_hundreds(api, tmp_path):
    name = R.GROW_CASE["name"]
    yc = R.reference(name)[2][2]
    assert yc.min() > 0.9 * R.GROW_CASE["T"]
    bar_check(api, tmp_path, name)


@pytest.mark.parametrize("name", names(R.INF_CASES))
def test_infinite_readings(api, tmp_path, name):
    """+inf in one feature of one row, -inf in another row's: the float64 definition keeps both rows finite (the gates of that step
    saturate; no weight of the planted column is 0, so no 0 . inf) and so must the kernel, within the bar; every other row keeps its bits"""
    clean = bar_check(api, tmp_path, name)
    got = bar_check(api, tmp_path, name, planted=True)
    ref = R.reference(name, planted=True)[2][0]
    hit = [r for r, _, _, _ in R.INF_AT]
    keep = np.setdiff1d(np.arange(clean.shape[0]), hit)
    assert same_bits(got[keep], clean[keep])
    assert np.isfinite(ref).all() and np.isfinite(got).all()
    assert R.verdict(got[hit], ref[hit]) <= 1.0 and not same_bits(got[hit], clean[hit])


def test_relu_on_generic_data(api, tmp_path):
    bar_check(api, tmp_path, R.RELU_CASE["name"])
