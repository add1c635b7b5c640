"""rnn_kernel<OP, LENS = true> (hip/rnn.hip) through the C ABI: per-row sequence_lens of LSTM / GRU / RNN (INTEGRATION.md section 2.6 "Padded
windows").  The rule: a row with length L gives what the same layer gives when run on that row's first L steps alone.

Two kinds of claim.  Against the FIXED-LENGTH kernel the claim is bit for bit and needs no tolerance: the arithmetic of a row and step is the
same and rows never mix, so a row of length L equals the model loaded with T = L on the row's prefix, is +0 behind L, and carries that
model's Y_h / Y_c.  Against the float64 reference (tests/recurrent_lens_ref.py, checked against torch's packing in
tests/test_recurrent_lens.py) the claim is the project bar, 1e-4 |ref| + 1e-6 through recurrent_ref.verdict, every element held to it."""
from __future__ import annotations

import contextlib

import numpy as np
import pytest

from infera_amd import onnx_writer as W
from tests import recurrent_lens_ref as RL
from tests import recurrent_ref as R

pytestmark = pytest.mark.gpu

OPS = {"LSTM": ("LSTM", {}), "GRU_lbr0": ("GRU", dict(linear_before_reset=0)), "GRU_lbr1": ("GRU", dict(linear_before_reset=1)), "RNN_tanh": ("RNN", dict(activation="Tanh"))}
TAILS = {"Y": "seq", "Y_h": "y_h", "Y_c": "y_c"}
LENS = dict(form="rank1", type=W.INT64)  # PyTorch's form: an int64 [N] input through Cast(to = INT32)


@pytest.fixture(scope="module")
def api(built):
    from infera_amd import capi

    assert capi.device_count() >= 1, capi.get_devices()
    return capi


@contextlib.contextmanager
def served(api, tmp_path, spec, output="Y", seq_lens=LENS, T=None, name="recurrent_lens", **kw):
    """one loaded model; with seq_lens every Recurrent step of its plan must carry the length column"""
    blob = W.recurrent_from_spec(spec, T=T, flat=True, tail=TAILS[output], seq_lens=seq_lens, **kw)
    api.load_model(name, W.write(str(tmp_path / (name + ".onnx")), blob))
    try:
        rec = [s for s in api.get_plan(name)["plan"]["steps"] if s["kind"] == "Recurrent"]
        assert len(rec) == len(spec["layers"]) and rec[-1]["output"] == output, rec
        assert all(("seq_lens" in s) == (seq_lens is not None) for s in rec), rec
        yield lambda table: api.predict(name, np.ascontiguousarray(table, np.float32))
    finally:
        api.unload_model(name)


def outputs_of(op):
    return ("Y", "Y_h", "Y_c") if op == "LSTM" else ("Y", "Y_h")


def lengths33(T, seed=0):
    """33 lengths: 0, every length 1 .. T, then draws from 0 .. T -- row 16 alone in its tile position, rows 32 a tile of one row"""
    rng = np.random.default_rng([seed, T])
    head = np.arange(0, T + 1)
    return np.concatenate([head, rng.integers(0, T + 1, 33 - head.size)])[:33].astype(np.int64)


def same_bits(got, ref):
    return got.shape == np.shape(ref) and np.array_equal(R.bits(got), R.bits(ref))


# ---- bits against the fixed-length kernel -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("direction", ["forward", "reverse", "bidirectional"])
@pytest.mark.parametrize("op", list(OPS))
@pytest.mark.parametrize("H", [1, 16, 144])
def test_rows_equal_the_fixed_length_model_bit_for_bit(api, tmp_path, H, op, direction):
    """H = 1 (padded units), 16 (one tile) and 144 (nine tiles on eight waves); F = 9 reaches the tail loop of the x_t fetch.  A non-zero
    initial state shows that a row of length 0 returns it."""
    T, F = 9, 9
    o, kw = OPS[op]
    spec = W.recurrent_spec(o, T=T, F=F, H=H, direction=direction, initial=0.5, **kw)
    D, last = spec["D"], spec["layers"][-1]
    x = R.inputs(33, T, F)
    lens = lengths33(T)
    assert set(lens) == set(range(T + 1))
    for output in outputs_of(o):
        with served(api, tmp_path, spec, output) as run:
            got = run(RL.with_lens(x, lens))
            all_T = run(RL.with_lens(x, np.full(33, T)))
        got = got.reshape(33, T, D * H) if output == "Y" else got.reshape(33, D * H)
        for L in range(1, T + 1):
            at = np.nonzero(lens == L)[0]
            with served(api, tmp_path, spec, output, seq_lens=None, T=L, name="recurrent_fixed") as fixed:
                want = fixed(x[at, :L].reshape(at.size, -1))
                if L == T:  # every length = T: the same model without sequence_lens, the whole table
                    assert same_bits(all_T, fixed(x.reshape(33, -1))), (output, "all lengths = T")
            if output == "Y":
                assert same_bits(got[at, :L], want.reshape(at.size, L, D * H)), (output, L)
                assert not R.bits(got[at, L:]).any(), (output, L, "not +0 behind the length")
            else:
                assert same_bits(got[at], want.reshape(at.size, D * H)), (output, L)
        zero = np.nonzero(lens == 0)[0]
        assert zero.size >= 1
        if output == "Y":
            assert not R.bits(got[zero]).any()
        else:
            init = last["h0"] if output == "Y_h" else last["c0"]
            assert same_bits(got[zero], np.tile(init.reshape(1, D * H), (zero.size, 1))), output


# ---- tile patterns against float64 --------------------------------------------------------------------------------------------------------

def patterns(T, n):
    """length patterns of an n-row call: every row 1; one whole tile of zeros (the step loop of that workgroup runs zero times; below 17 rows
    the only tile); descending from T; one long row last in a tile of short ones (the tile runs T steps for it); 1, 2, 3 and 4 frozen steps
    side by side (odd and even numbers of flips of the h double buffer behind a row's end)"""
    r = np.arange(n)
    rng = np.random.default_rng([T, n])
    zero_tile = rng.integers(0, T + 1, n)
    zero_tile[:16] = 0
    long_last = np.minimum(1, T) * np.ones(n, np.int64)
    long_last[min(15, n - 1)] = T
    return {"ones": np.ones(n, np.int64), "zero_tile": zero_tile, "descending": np.maximum(T - r, 0), "long_last": long_last,
            "frozen_parity": np.maximum(T - (r % 5), 0)}


@pytest.mark.parametrize("op", list(OPS))
@pytest.mark.parametrize("T,F", [(1, 1), (2, 17), (17, 1), (17, 17), (2, 1), (1, 17)], ids=lambda v: str(v))
def test_tile_patterns_against_float64(api, tmp_path, T, F, op):
    """bidirectional (both directions in one launch), H = 20 (two tiles, the second padded), rows 1, 16, 17 and 33"""
    o, kw = OPS[op]
    spec = W.recurrent_spec(o, T=T, F=F, H=20, direction="bidirectional", initial=0.5, **kw)
    x = R.inputs(33, T, F)
    worst = 0.0
    cases = {(n, name): lens for n in (1, 16, 17, 33) for name, lens in patterns(T, n).items()}
    refs = {k: RL.recurrent_rows(spec, x[:k[0]], lens) for k, lens in cases.items()}  # computed once, read by every output
    for i, output in enumerate(outputs_of(o)):
        with served(api, tmp_path, spec, output) as run:
            for (n, name), lens in cases.items():
                got = run(RL.with_lens(x[:n], lens))
                v = R.verdict(got, refs[(n, name)][i].reshape(got.shape))
                worst = max(worst, v)
                assert v <= 1.0, (output, n, name, v)
                if output == "Y":  # behind a row's length: written zeros, exactly
                    y = got.reshape(n, T, -1)
                    assert all(not R.bits(y[r, lens[r]:]).any() for r in range(n)), (n, name)
    print(f"tile patterns {op} T={T} F={F}: worst error / bar = {worst:.3f}")


@pytest.mark.parametrize("op", ["GRU_lbr0", "GRU_lbr1", "LSTM"])
def test_stacked_bidirectional_against_float64(api, tmp_path, op):
    """two layers: layer 2 reads layer 1's written zeros behind a row's length and its own lengths from the same column"""
    T, F, H = 9, 5, 24
    o, kw = OPS[op]
    spec = W.recurrent_spec(o, T=T, F=F, H=H, layers=2, direction="bidirectional", initial=0.5, **kw)
    x = R.inputs(33, T, F)
    lens = lengths33(T, seed=1)
    ref = RL.recurrent_rows(spec, x, lens)
    f32 = RL.recurrent_rows(spec, x, lens, np.float32)
    for i, output in enumerate(outputs_of(o)):
        assert R.verdict(f32[i], ref[i]) <= 0.25, output  # the case is a fair one for the bar: float32 itself stays within a quarter of it
        with served(api, tmp_path, spec, output) as run:
            got = run(RL.with_lens(x, lens))
        v = R.verdict(got, ref[i].reshape(got.shape))
        print(f"stacked {op} {output}: worst error / bar = {v:.3f}")
        assert v <= 1.0, (output, v)


# ---- padding is not read ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("op", list(OPS))
def test_padding_is_never_read(api, tmp_path, op):
    """NaN, +-inf and 3e38 at every t >= L of every row change no bit of any row (0 . NaN would be NaN: the step is not read at all)"""
    T, F, H = 9, 9, 40
    o, kw = OPS[op]
    spec = W.recurrent_spec(o, T=T, F=F, H=H, direction="bidirectional", **kw)
    x = R.inputs(33, T, F)
    lens = lengths33(T, seed=2)
    for output in outputs_of(o):
        with served(api, tmp_path, spec, output) as run:
            clean = run(RL.with_lens(RL.fill_padding(x, lens, 0.0), lens))
            assert np.isfinite(clean).all()
            for fill in (np.nan, np.inf, -np.inf, 3e38):
                assert same_bits(run(RL.with_lens(RL.fill_padding(x, lens, fill), lens)), clean), (output, fill)


# ---- bad lengths ----------------------------------------------------------------------------------------------------------------------------

def test_bad_lengths_fail_their_call_alone(api, tmp_path):
    T, F, H = 6, 3, 16
    spec = W.recurrent_spec("LSTM", T=T, F=F, H=H, direction="bidirectional")
    x = R.inputs(33, T, F)
    lens = lengths33(T, seed=3)
    with served(api, tmp_path, spec, "Y") as run:
        clean = run(RL.with_lens(x, lens))
        assert R.verdict(clean, RL.recurrent_rows(spec, x, lens)[0].reshape(clean.shape)) <= 1.0
        for bad in (-1.0, T + 1.0, np.nan):
            table = RL.with_lens(x, lens)
            table[20, -1] = bad
            with pytest.raises(api.InferaError, match=r"node 'rnn0' \(LSTM\): sequence_lens outside 0…T"):
                run(table)
            assert same_bits(run(RL.with_lens(x, lens)), clean), bad  # the next call on the model succeeds
        # the int64 length column arrives as f32 values, truncated toward zero: 2.9 is 2, -0.9 is 0, T + 0.9 is T
        table = RL.with_lens(x, lens)
        table[:3, -1] = (2.9, -0.9, T + 0.9)
        want = lens.copy()
        want[:3] = (2, 0, T)
        assert same_bits(run(table), run(RL.with_lens(x, want)))
        assert R.verdict(run(table), RL.recurrent_rows(spec, x, want)[0].reshape(clean.shape)) <= 1.0


# ---- call paths -------------------------------------------------------------------------------------------------------------------------------

def test_bits_independent_of_call_path(api, tmp_path):
    """33 rows in one call, as 16 + 17, column by column, and through the SQL surface: infera_predict over x_0 .. x_{T F - 1}, len"""
    from infera_amd import sqlharness as S

    S.lib()
    T, F, H = 6, 3, 16
    spec = W.recurrent_spec("GRU", T=T, F=F, H=H, direction="bidirectional")
    rng = np.random.default_rng(6)
    head = (rng.normal(0, 0.3, (2 * H, 1)).astype(np.float32), np.zeros(1, np.float32), None)
    x = R.inputs(33, T, F)
    lens = lengths33(T, seed=4)
    table = RL.with_lens(x, lens)
    path = W.write(str(tmp_path / "sql_lens.onnx"), W.recurrent_from_spec(spec, flat=True, tail="y_h", head=head, seq_lens=LENS))
    S.sql("infera_load_model", "sql_lens", path)
    try:
        ref = api.predict("sql_lens", table)
        yh = RL.recurrent_rows(spec, x, lens)[1]
        assert R.verdict(ref, yh @ head[0].astype(np.float64)) <= 1.0
        parts = np.concatenate([api.predict("sql_lens", np.ascontiguousarray(table[:16])), api.predict("sql_lens", np.ascontiguousarray(table[16:]))])
        assert same_bits(parts, ref)
        assert same_bits(api.predict_columns("sql_lens", [np.ascontiguousarray(table[:, j]) for j in range(table.shape[1])]), ref)
        cols = [np.ascontiguousarray(table[:, j]) for j in range(T * F)] + [lens.astype(np.int64)]
        got = np.asarray(S.sql("infera_predict", "sql_lens", *cols), np.float32).reshape(ref.shape)
        assert same_bits(got, ref)
    finally:
        S.sql("infera_unload_model", "sql_lens")
