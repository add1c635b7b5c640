"""ONNX LSTM / GRU / RNN at load time (no GPU): the forms exporters write and the plans they lower to, the row-axis aliases, the Y_h-only fold,
every form that is rejected with its reason, and the agreement of the two references the GPU tests use."""
from __future__ import annotations

import numpy as np
import pytest

from infera_amd import onnx_writer as W


@pytest.fixture(scope="module")
def api(built):
    from infera_amd import capi

    return capi


def _load(api, tmp_path, name, blob, select=""):
    p = W.write(str(tmp_path / f"{name}.onnx"), blob)
    api.load_model(name, p + select)
    try:
        return api.get_plan(name)["plan"], api.get_model_info(name)
    finally:
        api.unload_model(name)


G = {"LSTM": 4, "GRU": 3, "RNN": 1}
VARIANTS = [("LSTM", {}), ("GRU", dict(linear_before_reset=1)), ("GRU", dict(linear_before_reset=0)), ("RNN", dict(activation="Tanh")),
            ("RNN", dict(activation="Relu"))]
IDS = ["LSTM", "GRU_lbr1", "GRU_lbr0", "RNN_tanh", "RNN_relu"]


def _flops(op, T, F, H, D, layers=1):
    return sum(2 * T * D * G[op] * H * ((F if i == 0 else D * H) + H) for i in range(layers))


@pytest.mark.parametrize("op,kw", VARIANTS, ids=IDS)
def test_sequence_forms(api, tmp_path, op, kw):
    T, F, H = 24, 8, 64
    spec = W.recurrent_spec(op, T=T, F=F, H=H, **kw)
    for form in ("batch_first", "layout1"):  # forms 1 and 5: the Transposes / Squeeze are no step at all
        plan, info = _load(api, tmp_path, "m", W.recurrent_from_spec(spec, form=form))
        assert [s["kind"] for s in plan["steps"]] == ["Recurrent"]
        s = plan["steps"][0]
        assert (s["op"], s["T"], s["F"], s["H"], s["D"], s["output"]) == (op, T, F, H, 1, "Y")
        assert plan["input_shape"] == [-1, T, F] and plan["output_shape"] == [-1, T, H] and plan["flops_per_row"] == _flops(op, T, F, H, 1)
        assert info["input_shape"] == [-1, T, F] and info["output_shape"] == [-1, T, H]
        if op == "GRU":
            assert s["linear_before_reset"] == kw["linear_before_reset"]
        if op == "RNN":
            assert s["activation"] == kw["activation"]
    # form 6: a flat table
    plan, _ = _load(api, tmp_path, "m", W.recurrent_from_spec(spec, flat=True))
    assert plan["input_shape"] == [-1, T * F] and [s["kind"] for s in plan["steps"]] == ["Recurrent"]


@pytest.mark.parametrize("op,kw", VARIANTS, ids=IDS)
@pytest.mark.parametrize("layers,direction", [(1, "bidirectional"), (2, "forward"), (3, "forward"), (2, "bidirectional"), (3, "bidirectional"), (1, "reverse")])
def test_stacked_and_bidirectional(api, tmp_path, op, kw, layers, direction):
    T, F, H = 12, 4, 16
    spec = W.recurrent_spec(op, T=T, F=F, H=H, layers=layers, direction=direction, **kw)
    D = spec["D"]
    for form in ("batch_first", "layout1"):
        plan, _ = _load(api, tmp_path, "m", W.recurrent_from_spec(spec, form=form))
        assert [s["kind"] for s in plan["steps"]] == ["Recurrent"] * layers
        assert [(s["F"], s["D"], s["direction"]) for s in plan["steps"]] == [(F if i == 0 else D * H, D, direction) for i in range(layers)]
        assert plan["output_shape"] == [-1, T, D * H] and plan["flops_per_row"] == _flops(op, T, F, H, D, layers)


@pytest.mark.parametrize("op,kw", VARIANTS, ids=IDS)
def test_last_step_heads_and_the_fold(api, tmp_path, op, kw):
    T, F, H = 10, 3, 20
    spec = W.recurrent_spec(op, T=T, F=F, H=H, **kw)
    head = (np.zeros((H, 1), np.float32), np.zeros(1, np.float32), "Sigmoid")
    for form in ("batch_first", "layout1"):
        for tail, idx in (("last_gather", -1), ("last_gather", T - 1), ("last_slice", -1)):
            plan, _ = _load(api, tmp_path, "m", W.recurrent_from_spec(spec, form=form, tail=tail, last_index=idx, head=head))
            assert [s["kind"] for s in plan["steps"]] == ["Recurrent", "Dense"], (form, tail)
            assert plan["steps"][0]["output"] == "Y_h" and plan["output_shape"] == [-1, 1]  # only H values per row are stored
        plan, _ = _load(api, tmp_path, "m", W.recurrent_from_spec(spec, form=form, tail="y_h", head=head))
        assert [s["kind"] for s in plan["steps"]] == ["Recurrent", "Dense"] and plan["steps"][0]["output"] == "Y_h"
        # a step that is not the last one: the whole Y and a SliceCols
        plan, _ = _load(api, tmp_path, "m", W.recurrent_from_spec(spec, form=form, tail="last_gather", last_index=3))
        assert [s["kind"] for s in plan["steps"]] == ["Recurrent", "SliceCols"] and plan["steps"][0]["output"] == "Y"
        assert plan["output_shape"] == [-1, H]
    # bidirectional: the last step of Y is not the reverse direction's final state -- no fold; Y_h through Transpose + Reshape
    bi = W.recurrent_spec(op, T=T, F=F, H=H, direction="bidirectional", **kw)
    plan, _ = _load(api, tmp_path, "m", W.recurrent_from_spec(bi, tail="last_gather"))
    assert [s["kind"] for s in plan["steps"]] == ["Recurrent", "SliceCols"] and plan["output_shape"] == [-1, 2 * H]
    plan, _ = _load(api, tmp_path, "m", W.recurrent_from_spec(bi, tail="y_h", head=(np.zeros((2 * H, 3), np.float32), np.zeros(3, np.float32), None)))
    assert [s["kind"] for s in plan["steps"]] == ["Recurrent", "Dense"] and plan["output_shape"] == [-1, 3]


def test_pipeline_initial_state_and_named_outputs(api, tmp_path):
    T, F, H = 6, 4, 8
    spec = W.recurrent_spec("LSTM", T=T, F=F, H=H, initial=0.5, direction="bidirectional", layers=2)
    sc = (np.zeros(T * F, np.float32), np.full(T * F, 2.0, np.float32))
    for initial in ("const", "expand"):
        plan, _ = _load(api, tmp_path, "m", W.recurrent_from_spec(spec, scaler=sc, flat=True, initial=initial, tail="y_c"))
        assert [s["kind"] for s in plan["steps"]] == ["AffineChannel", "Recurrent", "Recurrent"]
        assert [s["output"] for s in plan["steps"][1:]] == ["Y", "Y_c"] and plan["output_shape"] == [-1, 2 * H]
    blob = W.recurrent_from_spec(spec, form="layout1", state_outputs=True)
    plan, info = _load(api, tmp_path, "m", blob, "#Y_h")
    assert plan["steps"][-1]["output"] == "Y_h" and info["output_shape"] == [-1, 2, H]
    # a time-major state [D, rows, H] cannot be served as it is: the reason names the way out
    with pytest.raises(api.InferaError, match=r"output 'Y_h' \[2,-1,8\] is time-major"):
        _load(api, tmp_path, "m", W.recurrent_from_spec(spec, state_outputs=True), "#Y_h")


def test_predict_without_gpu_fails_loudly(api, tmp_path):
    if api.device_count() > 0:
        return  # (with a GPU the call succeeds: tests/test_recurrent_gpu.py)
    p = W.write(str(tmp_path / "g.onnx"), W.recurrent_from_spec(W.recurrent_spec("GRU", T=4, F=2, H=8), flat=True))
    api.load_model("rnn_nogpu", p)
    try:
        with pytest.raises(api.InferaError, match="HIP backend unavailable"):
            api.predict("rnn_nogpu", np.zeros((3, 8), np.float32))
    finally:
        api.unload_model("rnn_nogpu")


# ---- rejections ------------------------------------------------------------------------------------------------------------------------

def _bad(op="LSTM", T=5, F=3, H=4, D=1, attrs=(), W_=None, R_=None, B_=None, extra_inputs=(), extra_inits=(), x_dims=None, nodes_before=(), x="Xt",
         inputs=None, tail=False):
    g = G[op]
    rng = np.random.default_rng(1)
    f32 = lambda *s: rng.normal(0, 0.1, s).astype(np.float32)  # noqa: E731
    inits = [W.tensor("W", f32(D, g * H, F) if W_ is None else W_), W.tensor("R", f32(D, g * H, H) if R_ is None else R_)]
    ins = [x, "W", "R"]
    if B_ is not None:
        inits.append(W.tensor("B", B_))
        ins.append("B")
    ins += list(extra_inputs)
    inits += list(extra_inits)
    nodes = [W.node("Transpose", ["X"], ["Xt"], [W.attr_ints("perm", [1, 0, 2])])] + list(nodes_before)
    nodes.append(W.node(op, ins if inputs is None else inputs, ["Y"], [W.attr_i("hidden_size", H)] + list(attrs), name="bad"))
    if tail:  # [T, 1, N, H] -> [N, T, H]: servable
        inits.append(W.tensor("tail_ax", np.array([1], np.int64)))
        nodes += [W.node("Squeeze", ["Y", "tail_ax"], ["Ys"]), W.node("Transpose", ["Ys"], ["Yo"], [W.attr_ints("perm", [1, 0, 2])])]
        return W.model("ok", nodes, inits, [W.value_info("X", ["N", T, F] if x_dims is None else x_dims)], [W.value_info("Yo", ["N", T, H])])
    return W.model("bad", nodes, inits, [W.value_info("X", ["N", T, F] if x_dims is None else x_dims)], [W.value_info("Y", [T, D, "N", H])])


def _z(*s):
    return np.zeros(s, np.float32)


REJECTED = [
    ("inputs", lambda: _bad(inputs=["Xt", "W"]), "needs the three inputs X, W, R"),
    ("W_not_const", lambda: _bad(inputs=["Xt", "Xt", "R"]), "W must be a constant f32 tensor"),
    ("W_shape", lambda: _bad(W_=_z(1, 16, 4)), r"W has shape \[1,16,4\], expected \[1,16,3\]"),
    ("R_shape", lambda: _bad(R_=_z(1, 12, 4)), r"R has shape \[1,12,4\], expected \[1,16,4\]"),
    ("B_shape", lambda: _bad(B_=_z(1, 16)), r"B has shape \[1,16\], expected \[1,32\]"),
    ("D_mismatch", lambda: _bad(attrs=[W.attr_s("direction", "bidirectional")]), r"W has shape \[1,16,3\], expected \[2,16,3\]"),
    ("sequence_lens", lambda: _bad(extra_inputs=["", "sl"], extra_inits=[W.tensor("sl", np.array([5, 5], np.int64))]), "sequence_lens"),
    ("initial_per_row", lambda: _bad(extra_inputs=["", "", "h0"], extra_inits=[W.tensor("h0", np.arange(8, dtype=np.float32).reshape(1, 2, 4))]),
     "initial_h differs per row"),
    # h0 = the first reading of every row: X[:, 0:1, :] ([N, 1, F], F == H) made time-major [1, N, H]
    ("initial_computed", lambda: _bad(F=4, nodes_before=[W.node("Slice", ["X", "h_b", "h_e", "h_ax"], ["h_rows"]),
                                                          W.node("Transpose", ["h_rows"], ["h0"], [W.attr_ints("perm", [1, 0, 2])])],
                                     extra_inputs=["", "", "h0"],
                                     extra_inits=[W.tensor("h_b", np.array([0], np.int64)), W.tensor("h_e", np.array([1], np.int64)),
                                                  W.tensor("h_ax", np.array([1], np.int64))]), "initial_h is computed from the rows"),
    ("peepholes", lambda: _bad(extra_inputs=["", "", "", "", "P"], extra_inits=[W.tensor("P", np.ones((1, 12), np.float32))]), "peepholes P that are not all zero"),
    ("input_forget", lambda: _bad(attrs=[W.attr_i("input_forget", 1)]), "input_forget = 1"),
    ("clip", lambda: _bad(attrs=[W.attr_f("clip", 3.0)]), "clip"),
    ("activations_lstm", lambda: _bad(attrs=[W.attr_strings("activations", ["HardSigmoid", "Tanh", "Tanh"])]), r"activations \(HardSigmoid, Tanh, Tanh\) other than the defaults"),
    ("activations_gru", lambda: _bad(op="GRU", attrs=[W.attr_strings("activations", ["Sigmoid", "Relu"])]), "other than the defaults"),
    ("activations_rnn", lambda: _bad(op="RNN", attrs=[W.attr_strings("activations", ["Sigmoid"])]), "other than the defaults"),
    ("activations_rnn_mixed", lambda: _bad(op="RNN", D=2, attrs=[W.attr_s("direction", "bidirectional"), W.attr_strings("activations", ["Relu", "Tanh"])]),
     "the same for both directions"),
    ("activation_alpha", lambda: _bad(attrs=[W.attr_floats("activation_alpha", [0.1])]), "activation_alpha"),
    ("direction", lambda: _bad(attrs=[W.attr_s("direction", "sideways")]), "direction 'sideways'"),
    ("H_cap", lambda: _bad(H=513, W_=_z(1, 4 * 513, 3), R_=_z(1, 4 * 513, 513)), "hidden_size 513 is above the cap of 512"),
    ("F_cap", lambda: _bad(F=1025, H=2, W_=_z(1, 8, 1025), R_=_z(1, 8, 2)), "input width 1025 is above the cap of 1024"),
    ("T_cap", lambda: _bad(T=4097), "sequence length 4097 is above the cap of 4096"),
    ("rows_first_X", lambda: _bad(x="X"), r"X must be \[T, rows, F\]"),
]


@pytest.mark.parametrize("what,build,why", REJECTED, ids=[r[0] for r in REJECTED])
def test_rejected_forms(api, tmp_path, what, build, why):
    with pytest.raises(api.InferaError, match=r"^ONNX error: node '\w+' \((\w+)\): .*" + why):
        _load(api, tmp_path, "bad", build())


def test_peepholes_of_zeros_and_empty_sequence_lens_load(api, tmp_path):
    blob = _bad(extra_inputs=["", "sl", "", "", "P"], extra_inits=[W.tensor("sl", np.zeros(0, np.int64)), W.tensor("P", _z(1, 12))], tail=True)
    plan, _ = _load(api, tmp_path, "ok", blob)
    assert [s["kind"] for s in plan["steps"]] == ["Recurrent"] and plan["steps"][0]["output"] == "Y" and plan["output_shape"] == [-1, 5, 4]


def test_symbolic_T_is_rejected(api, tmp_path):
    # a symbolic T can only come from the graph input, and the input check (older than these operators) refuses it before any node is read
    with pytest.raises(api.InferaError, match=r"^ONNX error: only the leading \(row/batch\) dimension of the input may be symbolic, got \[-1,-1,3\]$"):
        _load(api, tmp_path, "bad", _bad(x_dims=["N", "T", 3]))


def test_constant_of_shape_initial_state(api, tmp_path):
    spec = W.recurrent_spec("LSTM", T=6, F=4, H=8, initial=0.5)
    for L in spec["layers"]:
        L["h0"], L["c0"] = np.full((1, 8), 0.25, np.float32), np.zeros((1, 8), np.float32)
    for form in ("batch_first", "layout1"):
        plan, _ = _load(api, tmp_path, "fill", W.recurrent_from_spec(spec, form=form, initial="fill"))
        assert [s["kind"] for s in plan["steps"]] == ["Recurrent"]
    # a fill value that is not f32 is refused by name
    bad = _bad(nodes_before=[W.node("ConstantOfShape", ["cs"], ["h0"], [W.attr_tensor("value", W.tensor("", np.array([1], np.int64)))], name="fill")],
               extra_inputs=["", "", "h0"], extra_inits=[W.tensor("cs", np.array([1, 1, 4], np.int64))])
    with pytest.raises(api.InferaError, match=r"node 'fill' \(ConstantOfShape\): only an f32 fill value"):
        _load(api, tmp_path, "fill", bad)


def test_two_outputs_of_one_node(api, tmp_path):
    """Y (one step of it) and Y_h of the same LSTM both read: one Recurrent step per output that is read."""
    plan, _ = _load(api, tmp_path, "two", _two_outputs_model())
    assert [s["kind"] for s in plan["steps"]] == ["Recurrent", "Recurrent", "SliceCols", "BinaryAct"]
    assert [s["output"] for s in plan["steps"][:2]] == ["Y", "Y_h"] and plan["output_shape"] == [-1, 4]


def _two_outputs_model(T=5, F=3, H=4):
    spec = W.recurrent_spec("LSTM", T=T, F=F, H=H)
    L = spec["layers"][0]
    i64 = lambda n, v: W.tensor(n, np.asarray(v, dtype=np.int64))  # noqa: E731
    inits = [W.tensor("W", L["W"]), W.tensor("R", L["R"]), W.tensor("B", L["B"]), i64("ax0", [0]), i64("ax1", [1]), i64("first", 0)]
    nodes = [W.node("Transpose", ["X"], ["Xt"], [W.attr_ints("perm", [1, 0, 2])]),
             W.node("LSTM", ["Xt", "W", "R", "B"], ["Y", "Yh"], [W.attr_i("hidden_size", H)], name="both"),
             W.node("Squeeze", ["Y", "ax1"], ["Ys"]), W.node("Transpose", ["Ys"], ["seq"], [W.attr_ints("perm", [1, 0, 2])]),
             W.node("Gather", ["seq", "first"], ["y0"], [W.attr_i("axis", 1)]), W.node("Squeeze", ["Yh", "ax0"], ["hT"]),
             W.node("Add", ["y0", "hT"], ["out"])]
    return W.model("two", nodes, inits, [W.value_info("X", ["N", T, F])], [W.value_info("out", ["N", H])])


def _conv1d_slice_model(gather=False, C=3, L=8, M=8):
    """Conv1d -> one channel of it: a rank-3 activation that is NOT a sequence of time steps"""
    rng = np.random.default_rng(4)
    i64 = lambda n, v: W.tensor(n, np.asarray(v, dtype=np.int64))  # noqa: E731
    inits = [W.tensor("K", rng.normal(0, 0.3, (M, C, 3)).astype(np.float32)), i64("b", [4]), i64("e", [5]), i64("ax", [1]), i64("idx", 4)]
    pick = W.node("Gather", ["c", "idx"], ["out"], [W.attr_i("axis", 1)], name="pick") if gather else W.node("Slice", ["c", "b", "e", "ax"], ["out"], name="pick")
    nodes = [W.node("Conv", ["X", "K"], ["c"], [W.attr_ints("kernel_shape", [3])]), pick]
    return W.model("c1d", nodes, inits, [W.value_info("X", ["N", C, L])], [W.value_info("out", ["N", L - 2] if gather else ["N", 1, L - 2])])


def test_conv1d_channel_slice_lowers_as_before(api, tmp_path):
    """One channel of a Conv1d activation keeps the channel-slice path: a [N, 1, L] tensor, which keeps the plan out of the channel-quad
    layout; a Gather of it stays unsupported."""
    p = W.write(str(tmp_path / "c1d.onnx"), _conv1d_slice_model())
    api.load_model("c1d", p)
    try:
        full = api.get_plan("c1d")
    finally:
        api.unload_model("c1d")
    assert [s["kind"] for s in full["plan"]["steps"]] == ["Conv2d", "SliceCols"]
    assert full["plan"]["output_shape"] == [-1, 1, 6] and full["activation_layout"] == "NCHW"
    with pytest.raises(api.InferaError, match=r"node 'pick' \(Gather\): only constant data with constant indices is folded"):
        _load(api, tmp_path, "c1g", _conv1d_slice_model(gather=True))


def test_caps_from_the_inside(api, tmp_path):
    spec = W.recurrent_spec("GRU", T=2, F=1024, H=512, linear_before_reset=0)
    plan, _ = _load(api, tmp_path, "cap", W.recurrent_from_spec(spec))
    assert (plan["steps"][0]["F"], plan["steps"][0]["H"]) == (1024, 512)
    spec = W.recurrent_spec("RNN", T=4096, F=1, H=1)
    plan, _ = _load(api, tmp_path, "capT", W.recurrent_from_spec(spec, tail="last_gather"))
    assert plan["steps"][0]["T"] == 4096 and plan["steps"][0]["output"] == "Y_h"


def test_transposes_that_move_data_are_still_rejected(api, tmp_path):
    spec = W.recurrent_spec("LSTM", T=5, F=3, H=4)
    L = spec["layers"][0]
    inits = [W.tensor("W", L["W"]), W.tensor("R", L["R"])]
    # [N, T, F] -> (0, 2, 1): swaps time and features
    bad = W.model("t", [W.node("Transpose", ["X"], ["Y"], [W.attr_ints("perm", [0, 2, 1])], name="swap")], [], [W.value_info("X", ["N", 5, 3])],
                  [W.value_info("Y", ["N", 3, 5])])
    with pytest.raises(api.InferaError, match=r"node 'swap' \(Transpose\): .*would need data moved"):
        _load(api, tmp_path, "t", bad)
    # Y [T, 1, N, H] -> (2, 3, 0, 1): rows first, but H in front of T
    nodes = [W.node("Transpose", ["X"], ["Xt"], [W.attr_ints("perm", [1, 0, 2])]), W.node("LSTM", ["Xt", "W", "R"], ["Y"], [W.attr_i("hidden_size", 4)]),
             W.node("Transpose", ["Y"], ["Z"], [W.attr_ints("perm", [2, 3, 0, 1])], name="mix")]
    bad = W.model("t", nodes, inits, [W.value_info("X", ["N", 5, 3])], [W.value_info("Z", ["N", 4, 5, 1])])
    with pytest.raises(api.InferaError, match=r"node 'mix' \(Transpose\): .*would need data moved"):
        _load(api, tmp_path, "t", bad)
    # an operator that does not understand time-major values names the input
    # a rank-4 rows-first tensor is not touched by the alias rule: only the channel shuffle, as before
    bad = W.model("t", [W.node("Transpose", ["X"], ["Y"], [W.attr_ints("perm", [0, 1, 3, 2])], name="hw")], [], [W.value_info("X", ["N", 1, 4, 1])],
                  [W.value_info("Y", ["N", 1, 1, 4])])
    with pytest.raises(api.InferaError, match=r"node 'hw' \(Transpose\): on activations only the channel shuffle \(0,2,1,3,...\) keeps rows independent"):
        _load(api, tmp_path, "t", bad)
    nodes = nodes[:2] + [W.node("Relu", ["Y"], ["Z"], name="act")]
    bad = W.model("t", nodes, inits, [W.value_info("X", ["N", 5, 3])], [W.value_info("Z", [5, 1, "N", 4])])
    with pytest.raises(api.InferaError, match=r"node 'act' \(Relu\): input 'Y' \[5,1,-1,4\] is time-major"):
        _load(api, tmp_path, "t", bad)
    # merging the row axis into another one
    i64 = W.tensor("shape", np.array([-1, 4], np.int64))
    nodes = nodes[:2] + [W.node("Reshape", ["Y", "shape"], ["Z"], name="merge")]
    bad = W.model("t", nodes, inits + [i64], [W.value_info("X", ["N", 5, 3])], [W.value_info("Z", ["M", 4])])
    with pytest.raises(api.InferaError, match=r"node 'merge' \(Reshape\)"):
        _load(api, tmp_path, "t", bad)


# ---- the two references of tests/test_recurrent_gpu.py agree ---------------------------------------------------------------------------------

def test_references_agree():
    torch = pytest.importorskip("torch")
    import importlib.util
    import os

    from tests import recurrent_ref

    spec_ = importlib.util.spec_from_file_location("recurrent_gpu_refs", os.path.join(os.path.dirname(__file__), "test_recurrent_gpu.py"))
    g = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(g)
    for op, relu in g.OPS:
        for T, F, H, layers, D in [(9, 5, 12, 1, 1), (7, 3, 5, 2, 2), (1, 4, 16, 1, 2)]:
            m = g.torch_module(op, F, H, layers, D, relu)
            spec = W.torch_recurrent_spec(m)
            x = g._x(11, T, F)
            y_t, h_t = g.torch_ref(m, x, torch.float64)
            spec64 = dict(spec, layers=[{k: (v if v is None else np.asarray(v)) for k, v in L.items()} for L in spec["layers"]])
            y_n, h_n, _ = recurrent_ref.recurrent(spec64, x)
            # (the ONNX weights are the module's float32 parameters, which float64 holds exactly)
            assert np.max(np.abs(y_t - y_n)) <= 1e-12 and np.max(np.abs(h_t - h_n)) <= 1e-12, (op, relu, T, F, H, layers, D)
