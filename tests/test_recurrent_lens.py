"""Per-row sequence_lens of LSTM / GRU / RNN at load time (no GPU; INTEGRATION.md section 2.6 "Padded windows"): every form the writer gives
loads to one Recurrent step per read output that names its length column, the tracing nodes and the length input emit nothing, the
last-step fold stays away from a layer with lengths, every refused form names its node, the writer's default bytes are unchanged, and the
reference the GPU tests use (tests/recurrent_lens_ref.py) agrees with torch's pack_padded_sequence in float64."""
from __future__ import annotations

import numpy as np
import pytest

from infera_amd import onnx_writer as W
from tests import recurrent_lens_ref as RL
from tests import recurrent_ref as R


@pytest.fixture(scope="module")
def api(built):
    from infera_amd import capi

    return capi


def _load(api, tmp_path, blob, select=""):
    p = W.write(str(tmp_path / "lens.onnx"), blob)
    api.load_model("lens", p + select)
    try:
        return api.get_plan("lens")["plan"], api.get_model_info("lens")
    finally:
        api.unload_model("lens")


T, F, H = 6, 3, 8
TF = T * F
# (seq_lens of recurrent_from_spec, columns of the whole input, the length's column)
FORMS = {
    "rank1_int32": (dict(form="rank1", type=W.INT32), TF + 1, TF),
    "rank1_int64_cast": (dict(form="rank1", type=W.INT64), TF + 1, TF),  # PyTorch: Cast(lengths, INT32)
    "col_squeeze": (dict(form="col", squeeze="squeeze"), TF + 1, TF),
    "col_reshape": (dict(form="col", squeeze="reshape"), TF + 1, TF),
    "col_flatten": (dict(form="col", squeeze="flatten"), TF + 1, TF),
    "col_int32_no_cast": (dict(form="col", type=W.INT32), TF + 1, TF),
    "wide_slice": (dict(form="wide", k=3, col=1, pick="slice"), TF + 3, TF + 1),
    "wide_slice_reshape": (dict(form="wide", k=3, col=0, pick="slice", squeeze="reshape"), TF + 3, TF),
    "wide_gather": (dict(form="wide", k=3, col=2, pick="gather"), TF + 3, TF + 2),
    "wide_int32_gather": (dict(form="wide", k=2, col=1, pick="gather", type=W.INT32), TF + 2, TF + 1),
    "single_float_cast": (dict(form="single"), TF + 1, TF),
}


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("op", ["LSTM", "GRU", "RNN"])
def test_forms_load(api, tmp_path, op, form):
    sl, width, col = FORMS[form]
    spec = W.recurrent_spec(op, T=T, F=F, H=H, layers=2, direction="bidirectional")
    for tail, outputs in (("seq", ["Y", "Y"]), ("y_h", ["Y", "Y_h"])) + ((("y_c", ["Y", "Y_c"]),) if op == "LSTM" else ()):
        plan, info = _load(api, tmp_path, W.recurrent_from_spec(spec, tail=tail, seq_lens=sl))
        steps = plan["steps"]
        rec = [s for s in steps if s["kind"] == "Recurrent"]
        # one step per read output of every layer; what is not one is the SliceCols that cuts the readings out of the input buffer
        assert [s["output"] for s in rec] == outputs, steps
        assert all(s["seq_lens"] == {"src_col": col} for s in rec), steps
        others = [s for s in steps if s["kind"] != "Recurrent"]
        assert [s["kind"] for s in others] == ["SliceCols"] and ("input:X" in others[0]["origin"] or "sl_readings" in others[0]["origin"]), steps
        assert not any("len" in s["origin"] or "meta" in s["origin"] or "sl_" in s["origin"] for s in rec), steps
        assert plan["input_shape"] == [-1, width] and info["input_shape"] == [-1, width]
        assert plan["output_shape"] == ([-1, T, 2 * H] if tail == "seq" else [-1, 2 * H])


def test_state_outputs_share_one_length_column(api, tmp_path):
    """Y, Y_h and Y_c of one LSTM, all read: three steps, one column; the length as a second graph output that is not served is no reader"""
    spec = W.recurrent_spec("LSTM", T=T, F=F, H=H)
    blob = W.recurrent_from_spec(spec, form="layout1", state_outputs=True, seq_lens=dict(form="rank1", extra_output=True))
    for select, want in (("", ["Y"]), ("#Y_h", ["Y_h"]), ("#Y_c", ["Y_c"])):
        plan, _ = _load(api, tmp_path, blob, select)
        rec = [s for s in plan["steps"] if s["kind"] == "Recurrent"]
        assert [s["output"] for s in rec] == want and all(s["seq_lens"] == {"src_col": TF} for s in rec), plan["steps"]


def test_last_step_is_not_folded_behind_lengths(api, tmp_path):
    """Y[T - 1] of a short row is 0, not its Y_h: the Slice / Gather of the last step stays a SliceCols; without lengths it still folds"""
    spec = W.recurrent_spec("GRU", T=T, F=F, H=H)
    for tail in ("last_slice", "last_gather"):
        plan, _ = _load(api, tmp_path, W.recurrent_from_spec(spec, flat=True, tail=tail, seq_lens=dict(form="rank1")))
        kinds = [(s["kind"], s.get("output")) for s in plan["steps"]]
        assert kinds == [("SliceCols", None), ("Recurrent", "Y"), ("SliceCols", None)], kinds
        assert plan["output_shape"] == [-1, H]
        plan, _ = _load(api, tmp_path, W.recurrent_from_spec(spec, flat=True, tail=tail))
        assert [(s["kind"], s.get("output")) for s in plan["steps"]] == [("Recurrent", "Y_h")]


REFUSED = {
    "activation": (dict(source="activation"), {}, r"node 'rnn0' \(LSTM\): unsupported operator form: .*'len_a' is not a column range of a graph input \(a length computed from activations"),
    "reduce_sum_of_mask": (dict(source="reduce_sum"), {}, r"node 'rnn0' \(LSTM\): unsupported operator form: sequence_lens computed by the ReduceSum 'ReduceSum:sl_sum'"),
    "float16_source": (dict(form="single", type=W.FLOAT16), {}, r"node 'rnn0' \(LSTM\): unsupported operator form: sequence_lens taken from a float16 graph input"),
    "time_major": (dict(source="transpose"), {}, r"node 'rnn0' \(LSTM\): unsupported operator form: a time-major sequence_lens source \(the Transpose 'Transpose:sl_transpose'"),
    "two_columns": (dict(source="two_cols"), {}, r"node 'rnn0' \(LSTM\): unsupported operator form: sequence_lens traced to 2 columns of a graph input as \[-1,2\]; only one length per row"),
    "float_without_cast": (dict(form="col", type=W.FLOAT, cast=False), {}, r"node 'rnn0' \(LSTM\): unsupported operator form: sequence_lens read from a float graph input without a Cast"),
    "feeds_outside": (dict(form="col", shared=True), dict(tail="y_h"),
                      r"node 'sl_cast' \(Cast\): unsupported operator form: this node of a sequence_lens sub-graph also feeds nodes outside"),
}


@pytest.mark.parametrize("what", list(REFUSED))
def test_refused_forms(api, tmp_path, what):
    sl, kw, why = REFUSED[what]
    spec = W.recurrent_spec("LSTM", T=T, F=F, H=H)
    with pytest.raises(api.InferaError, match=r"^ONNX error: " + why):
        _load(api, tmp_path, W.recurrent_from_spec(spec, seq_lens=sl, **kw))


def test_constant_sequence_lens_keeps_its_refusal(api, tmp_path):
    """a constant cannot match a symbolic row count: refused in pack_recurrent's words, as tests/test_recurrent.py expects"""
    rng = np.random.default_rng(1)
    inits = [W.tensor("W", rng.normal(0, 0.1, (1, 16, 3)).astype(np.float32)), W.tensor("R", rng.normal(0, 0.1, (1, 16, 4)).astype(np.float32)),
             W.tensor("sl", np.array([5, 5], np.int32), int32_data=True)]
    nodes = [W.node("Transpose", ["X"], ["Xt"], [W.attr_ints("perm", [1, 0, 2])]),
             W.node("LSTM", ["Xt", "W", "R", "", "sl"], ["Y"], [W.attr_i("hidden_size", 4)], name="bad")]
    blob = W.model("bad", nodes, inits, [W.value_info("X", ["N", 5, 3])], [W.value_info("Y", [5, 1, "N", 4])])
    with pytest.raises(api.InferaError, match=r"^ONNX error: node 'bad' \(LSTM\): unsupported operator form: sequence_lens \(per-row sequence lengths\)$"):
        _load(api, tmp_path, blob)


def test_rank1_float_input_keeps_the_multi_input_refusal(api, tmp_path):
    spec = W.recurrent_spec("LSTM", T=T, F=F, H=H)
    with pytest.raises(api.InferaError, match=r"^ONNX error: multi-input models need f32 \[rows, k\] inputs with one common leading dimension; input 'len' is \[-1\]$"):
        _load(api, tmp_path, W.recurrent_from_spec(spec, seq_lens=dict(form="rank1", type=W.FLOAT, cast=False)))


def test_defaults_write_the_same_bytes_and_plans(api, tmp_path):
    for op, kw in (("LSTM", {}), ("GRU", dict(layers=2, direction="bidirectional")), ("RNN", dict(direction="reverse", initial=0.5))):
        spec = W.recurrent_spec(op, T=T, F=F, H=H, **kw)
        for form_kw in (dict(), dict(flat=True, tail="y_h"), dict(form="layout1", tail="last_slice", state_outputs=True)):
            assert W.recurrent_from_spec(spec, **form_kw) == W.recurrent_from_spec(spec, seq_lens=None, **form_kw)
            plan, _ = _load(api, tmp_path, W.recurrent_from_spec(spec, **form_kw))
            assert not any("seq_lens" in s for s in plan["steps"]), plan["steps"]
            lens_plan, _ = _load(api, tmp_path, W.recurrent_from_spec(spec, **dict(form_kw, seq_lens=dict(form="rank1"))))
            assert plan["flops_per_row"] == lens_plan["flops_per_row"]  # an upper bound for padded rows, as for padded attention


# ---- the reference against torch ---------------------------------------------------------------------------------------------------------

TORCH_CASES = [("LSTM", {}), ("GRU", {}), ("RNN", dict(nonlinearity="tanh")), ("RNN", dict(nonlinearity="relu"))]


@pytest.mark.parametrize("direction", ["forward", "reverse", "bidirectional"])
@pytest.mark.parametrize("op,kw", TORCH_CASES, ids=["LSTM", "GRU", "RNN_tanh", "RNN_relu"])
def test_reference_agrees_with_torch_packing(op, kw, direction, layers=2):
    """pad_packed_sequence(m(pack_padded_sequence(x, lens))) in float64 against recurrent_rows, lengths 1 .. T (torch refuses 0), two layers.
    torch has no reverse-only layer: "reverse" is the forward module on each row's flipped prefix, flipped back."""
    import torch
    from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

    torch.manual_seed(5)
    Tt, Ft, Ht, N = 7, 3, 5, 11
    bi = direction == "bidirectional"
    mod = getattr(torch.nn, op)(Ft, Ht, num_layers=1 if direction == "reverse" else layers, batch_first=True, bidirectional=bi, **kw).double()
    rng = np.random.default_rng(9)
    lens = np.concatenate([np.arange(1, Tt + 1), rng.integers(1, Tt + 1, N - Tt)])
    x = rng.normal(0, 1, (N, Tt, Ft))
    with torch.no_grad():
        for p in mod.parameters():  # weights that float32 holds exactly, so that the spec (float32) and the module (float64) are one model
            p.copy_(p.float().double())
        spec = W.torch_recurrent_spec(mod)
        spec["T"] = Tt
        if direction == "reverse":
            spec["direction"] = "reverse"
            xin = np.zeros_like(x)
            for r, L in enumerate(lens):
                xin[r, :L] = x[r, :L][::-1]
        else:
            xin = x
        packed = pack_padded_sequence(torch.from_numpy(xin), torch.from_numpy(lens), batch_first=True, enforce_sorted=False)
        out, state = mod(packed)
        y_t = pad_packed_sequence(out, batch_first=True, total_length=Tt)[0].numpy()
        h_t = (state[0] if op == "LSTM" else state).numpy()
        c_t = state[1].numpy() if op == "LSTM" else None
    if direction == "reverse":
        for r, L in enumerate(lens):
            y_t[r, :L] = y_t[r, :L][::-1].copy()
    D = spec["D"]
    last = lambda s: np.concatenate([s[-D + d] for d in range(D)], axis=1)  # noqa: E731  (h_n is [layers * D, N, H])
    y, yh, yc = RL.recurrent_rows(spec, x, lens)
    assert np.abs(y - y_t).max() <= 1e-12 and np.abs(yh - last(h_t)).max() <= 1e-12
    if op == "LSTM":
        assert np.abs(yc - last(c_t)).max() <= 1e-12
    for r, L in enumerate(lens):
        assert not y[r, L:].any() and not y_t[r, L:].any()
    # what lies behind a row's length is not touched
    y2, yh2, _ = RL.recurrent_rows(spec, RL.fill_padding(x, lens, np.nan), lens)
    assert np.array_equal(y2, y) and np.array_equal(yh2, yh)


def test_reference_zero_length_is_the_initial_state():
    spec = W.recurrent_spec("LSTM", T=4, F=2, H=3, layers=2, direction="bidirectional", initial=0.5)
    x = R.inputs(3, 4, 2)
    y, yh, yc = RL.recurrent_rows(spec, x, [0, 4, 0])
    last = spec["layers"][-1]
    assert not y[0].any() and not y[2].any() and y[1].all()
    assert np.array_equal(yh[0], last["h0"].reshape(-1).astype(np.float64)) and np.array_equal(yc[2], last["c0"].reshape(-1).astype(np.float64))
    full = R.recurrent(spec, x[1:2])
    assert np.array_equal(y[1], full[0][0]) and np.array_equal(yh[1], full[1][0]) and np.array_equal(yc[1], full[2][0])
    assert RL.with_lens(x, [0, 4, 0]).shape == (3, 9) and RL.with_lens(x, [0, 4, 0])[1, 8] == 4.0
