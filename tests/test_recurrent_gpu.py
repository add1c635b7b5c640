"""ONNX LSTM / GRU / RNN on the GPU through the C ABI (hip/rnn.hip): parity with torch.nn in float64 and with a float64 numpy restatement of the
operator specification, at the project's bar |hip - ref| <= 1e-4 |ref| + 1e-6 on every element, and bit-identity between the call paths."""
from __future__ import annotations

import numpy as np
import pytest

from infera_amd import onnx_writer as W
from tests.recurrent_ref import recurrent as np_recurrent  # the float64 restatement of the ONNX operator specification

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 1e-6


@pytest.fixture(scope="module")
def api(built):
    from infera_amd import capi

    assert capi.device_count() >= 1, capi.get_devices()
    return capi


def w_scale(op, relu, shape):
    """Cases in which float32 itself (torch on the CPU) would use more than a quarter of the bar get smaller weights, as measured on
    the CPU (profiles/r10_recurrent.txt): the 1024-term dot products of the cap shape, and the two-layer bidirectional tanh RNN."""
    if shape[2] >= 512:
        return 0.25
    return 0.5 if (op == "RNN" and not relu and shape == (96, 4, 128, 2, 2)) else 1.0


def torch_module(op, F, H, layers, D, relu=False, seed=5, scale=1.0):
    torch.manual_seed(seed)
    kw = dict(input_size=F, hidden_size=H, num_layers=layers, bidirectional=D == 2, batch_first=True)
    m = torch.nn.RNN(nonlinearity="relu" if relu else "tanh", **kw) if op == "RNN" else getattr(torch.nn, op)(**kw)
    if scale != 1.0:
        with torch.no_grad():
            for p in m.parameters():
                p.mul_(scale)
    if relu:  # keep the recurrence contractive: spectral norm of every R below 1
        with torch.no_grad():
            for name, p in m.named_parameters():
                if name.startswith("weight_hh"):
                    p.mul_(0.9 / max(1.0, float(torch.linalg.matrix_norm(p, 2))))
    return m


def torch_ref(m, x, dtype):
    mm = type(m)(**{k: getattr(m, k) for k in ("input_size", "hidden_size", "num_layers", "bidirectional", "batch_first")},
                 **({"nonlinearity": m.nonlinearity} if isinstance(m, torch.nn.RNN) else {})).to(dtype)
    mm.load_state_dict({k: v.to(dtype) for k, v in m.state_dict().items()})
    with torch.no_grad():
        y, st = mm(torch.from_numpy(x).to(dtype))
    hn = st[0] if isinstance(st, tuple) else st
    N = x.shape[0]
    D, H = (2 if m.bidirectional else 1), m.hidden_size
    yh = hn[-D:].permute(1, 0, 2).reshape(N, D * H)
    return y.double().numpy(), yh.double().numpy()


def worst_ratio(got, ref):
    """max over the elements of |got - ref| / (RTOL |ref| + ATOL): <= 1 passes the bar."""
    return float(np.max(np.abs(np.asarray(got, np.float64) - ref) / (RTOL * np.abs(ref) + ATOL)))


def _model(spec, **kw):
    """infera_predict hands the model a rank-2 [rows, cols] table, so the models take the flat [N, T*F] input and reshape it themselves"""
    return W.recurrent_from_spec(spec, flat=True, **kw)


def _predict(api, tmp_path, blob, x, name="rnn", select=""):
    p = W.write(str(tmp_path / f"{name}.onnx"), blob)
    api.load_model(name, p + select)
    try:
        return api.predict(name, x.reshape(x.shape[0], -1))
    finally:
        api.unload_model(name)


def _x(rows, T, F, seed=3):
    return np.random.default_rng(seed).normal(0, 1, (rows, T, F)).astype(np.float32)


# (T, F, H, layers, D): the issue's shapes, the caps at a small T, and T = 1
SHAPES = [(24, 8, 64, 1, 1), (50, 1, 32, 2, 1), (96, 4, 128, 2, 2), (256, 16, 64, 1, 1), (12, 30, 100, 1, 1), (7, 3, 5, 1, 2), (3, 1024, 512, 1, 1),
          (1, 8, 64, 1, 1)]
OPS = [("LSTM", False), ("GRU", False), ("RNN", False), ("RNN", True)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("op,relu", OPS, ids=["LSTM", "GRU", "RNN_tanh", "RNN_relu"])
def test_parity_with_torch_float64(api, tmp_path, op, relu, shape):
    T, F, H, layers, D = shape
    m = torch_module(op, F, H, layers, D, relu, scale=w_scale(op, relu, shape))
    spec = W.torch_recurrent_spec(m)
    x = _x(17 if H >= 512 else 67, T, F)
    ref_y, ref_h = torch_ref(m, x, torch.float64)
    # what fp32 itself costs on these inputs: at most a quarter of the bar, else the case is not a fair one
    f32_y, _ = torch_ref(m, x, torch.float32)
    r32 = worst_ratio(f32_y, ref_y)
    got = _predict(api, tmp_path, _model(spec, T=T), x)
    rk = worst_ratio(got.reshape(ref_y.shape), ref_y)
    print(f"\nratio {op}{'_relu' if relu else ''} {shape}: torch-f32 {r32:.4f} kernel {rk:.4f}")
    assert r32 <= 0.25, r32
    assert rk <= 1.0, rk
    got_h = _predict(api, tmp_path, _model(spec, T=T, tail="y_h"), x)
    assert worst_ratio(got_h, ref_h) <= 1.0


NP_CASES = [("GRU", dict(linear_before_reset=0)), ("GRU", dict(linear_before_reset=0, direction="bidirectional", layers=2)),
            ("LSTM", dict(direction="reverse")), ("GRU", dict(direction="reverse")), ("RNN", dict(direction="reverse")),
            ("LSTM", dict(initial=0.5)), ("LSTM", dict(initial=0.5, direction="bidirectional", layers=2)), ("GRU", dict(initial=0.5)),
            ("RNN", dict(initial=0.5, bias=False))]


@pytest.mark.parametrize("op,kw", NP_CASES, ids=lambda v: v if isinstance(v, str) else "_".join(f"{k}{x}" for k, x in v.items()))
@pytest.mark.parametrize("form,initial", [("batch_first", "const"), ("layout1", "expand")])
def test_parity_with_numpy_restatement(api, tmp_path, op, kw, form, initial):
    spec = W.recurrent_spec(op, T=20, F=6, H=40, **kw)
    x = _x(33, 20, 6, seed=8)
    y, yh, yc = np_recurrent(spec, x)
    got = _predict(api, tmp_path, _model(spec, form=form, initial=initial), x)
    assert worst_ratio(got.reshape(y.shape), y) <= 1.0
    got = _predict(api, tmp_path, _model(spec, form=form, initial=initial, tail="y_h"), x)
    assert worst_ratio(got, yh) <= 1.0
    if op == "LSTM":
        got = _predict(api, tmp_path, _model(spec, form=form, initial=initial, tail="y_c"), x)
        assert worst_ratio(got, yc) <= 1.0


@pytest.mark.parametrize("rows", [1, 17, 2048, 2049, (1 << 18) + 5])
def test_row_counts(api, tmp_path, rows):
    m = torch_module("LSTM", 4, 32, 1, 1)
    x = _x(rows, 6, 4, seed=rows % 97)
    ref_y, _ = torch_ref(m, x, torch.float64)
    got = _predict(api, tmp_path, _model(W.torch_recurrent_spec(m), T=6), x)
    assert got.shape == (rows, 6 * 32)
    assert worst_ratio(got.reshape(ref_y.shape), ref_y) <= 1.0


def test_heads_and_pipeline_forms(api, tmp_path):
    T, F, H = 12, 5, 24
    rng = np.random.default_rng(2)
    x = _x(100, T, F, seed=4)
    off, sc = rng.normal(0, 1, T * F).astype(np.float32), rng.uniform(0.5, 2, T * F).astype(np.float32)
    xs = ((x.reshape(100, -1).astype(np.float64) - off) * sc).reshape(100, T, F)
    Wd, bd = rng.normal(0, 0.3, (H, 1)).astype(np.float32), rng.normal(0, 0.1, 1).astype(np.float32)
    for op in ("LSTM", "GRU"):
        spec = W.recurrent_spec(op, T=T, F=F, H=H)
        y, yh, _ = np_recurrent(spec, xs)
        ref = 1 / (1 + np.exp(-(y[:, -1] @ Wd.astype(np.float64) + bd)))
        for tail in ("last_gather", "last_slice", "y_h"):
            got = _predict(api, tmp_path, _model(spec, scaler=(off, sc), tail=tail, head=(Wd, bd, "Sigmoid")), x.reshape(100, -1))
            assert got.shape == (100, 1) and worst_ratio(got, ref) <= 1.0, (op, tail)


def test_bits_independent_of_call_path(api, tmp_path):
    T, F, H, rows = 10, 6, 48, 20000
    x = _x(rows, T, F, seed=9)
    flat = np.ascontiguousarray(x.reshape(rows, T * F))
    spec = W.recurrent_spec("LSTM", T=T, F=F, H=H, seed=3)
    p = W.write(str(tmp_path / "rep.onnx"), W.recurrent_from_spec(spec, flat=True, state_outputs=True, form="layout1"))
    api.load_model("rep", p)
    api.load_model("rep_h", p + "#Y_h")
    api.load_model("rep_g", W.write(str(tmp_path / "rep_g.onnx"), W.recurrent_from_spec(spec, flat=True, tail="last_gather")))
    api.load_model("rep_r", W.write(str(tmp_path / "rep_r.onnx"), W.recurrent_from_spec(dict(spec, direction="reverse"), flat=True, state_outputs=True, form="layout1")))
    api.load_model("rep_rh", str(tmp_path / "rep_r.onnx") + "#Y_h")
    try:
        assert api.get_plan("rep_g")["plan"]["steps"][0]["output"] == "Y_h"
        ref = api.predict("rep", flat).reshape(rows, T, H)
        for step in (1, 7, 2048, 2049):  # a row alone, a row in its batch, chunk boundaries
            n = rows if step > 7 else 300
            parts = [api.predict("rep", flat[i:min(i + step, n)]) for i in range(0, n, step)]
            assert np.array_equal(np.concatenate(parts).reshape(n, T, H), ref[:n]), step
        cols = [np.ascontiguousarray(flat[:, j]) for j in range(T * F)]
        assert np.array_equal(api.predict_columns("rep", cols).reshape(rows, T, H), ref)  # column-major staged == row-major
        api.register_host_memory(flat)
        try:
            assert np.array_equal(api.predict("rep", flat).reshape(rows, T, H), ref)  # zero-copy == staged
        finally:
            api.unregister_host_memory(flat)
        dev = api.device_ordinal(0)
        d_in, d_out = api.DeviceBuffer(dev, flat.nbytes), api.DeviceBuffer(dev, rows * T * H * 4)
        d_in.upload(flat)
        api.predict_device("rep", d_in, rows, T * F, d_out)
        assert np.array_equal(d_out.download((rows, T, H)), ref)  # device-resident scan == host chunks
        yh = api.predict("rep_h", flat)
        assert np.array_equal(yh.reshape(rows, H), ref[:, -1])  # Y_h == Y[T-1] forward
        assert np.array_equal(api.predict("rep_g", flat), ref[:, -1])  # the Y_h-only fold == the last step of the full Y
        assert np.array_equal(api.predict("rep_rh", flat).reshape(rows, H), api.predict("rep_r", flat).reshape(rows, T, H)[:, 0])  # Y_h == Y[0] reverse
        assert np.array_equal(api.predict_from_blob("rep", x[3].tobytes()).reshape(T, H), ref[3])
    finally:
        for n in ("rep", "rep_h", "rep_g", "rep_r", "rep_rh"):
            api.unload_model(n)


def test_constant_of_shape_state_and_two_outputs(api, tmp_path):
    spec = W.recurrent_spec("LSTM", T=9, F=4, H=24, initial=0.5)
    for L in spec["layers"]:
        L["h0"], L["c0"] = np.full((1, 24), 0.25, np.float32), np.full((1, 24), -0.5, np.float32)
    x = _x(50, 9, 4, seed=15)
    y, _, yc = np_recurrent(spec, x)
    for form in ("batch_first", "layout1"):
        assert worst_ratio(_predict(api, tmp_path, _model(spec, form=form, initial="fill"), x).reshape(y.shape), y) <= 1.0
        assert worst_ratio(_predict(api, tmp_path, _model(spec, form=form, initial="fill", tail="y_c"), x), yc) <= 1.0
    # Y (its first step) + Y_h of one node, both read
    spec = W.recurrent_spec("LSTM", T=5, F=3, H=4)
    L = spec["layers"][0]
    i64 = lambda n, v: W.tensor(n, np.asarray(v, dtype=np.int64))  # noqa: E731
    inits = [W.tensor("W", L["W"]), W.tensor("R", L["R"]), W.tensor("B", L["B"]), i64("ax0", [0]), i64("ax1", [1]), i64("first", 0), i64("s3", [-1, 5, 3])]
    nodes = [W.node("Reshape", ["X", "s3"], ["X3"]), W.node("Transpose", ["X3"], ["Xt"], [W.attr_ints("perm", [1, 0, 2])]),
             W.node("LSTM", ["Xt", "W", "R", "B"], ["Y", "Yh"], [W.attr_i("hidden_size", 4)], name="both"),
             W.node("Squeeze", ["Y", "ax1"], ["Ys"]), W.node("Transpose", ["Ys"], ["seq"], [W.attr_ints("perm", [1, 0, 2])]),
             W.node("Gather", ["seq", "first"], ["y0"], [W.attr_i("axis", 1)]), W.node("Squeeze", ["Yh", "ax0"], ["hT"]), W.node("Add", ["y0", "hT"], ["out"])]
    blob = W.model("two", nodes, inits, [W.value_info("X", ["N", 15])], [W.value_info("out", ["N", 4])])
    x = _x(40, 5, 3, seed=16)
    y, yh, _ = np_recurrent(spec, x)
    assert worst_ratio(_predict(api, tmp_path, blob, x), y[:, 0] + yh) <= 1.0


def test_conv1d_channel_slice_is_still_the_channel(api, tmp_path):
    """A rank-3 activation that is not a sequence: channel 4 of a Conv1d output (a plan without recurrent layers computes what it did)."""
    C, L, M = 3, 8, 8
    rng = np.random.default_rng(4)
    K = rng.normal(0, 0.3, (M, C, 3)).astype(np.float32)
    i64 = lambda n, v: W.tensor(n, np.asarray(v, dtype=np.int64))  # noqa: E731
    nodes = [W.node("Conv", ["X", "K"], ["c"], [W.attr_ints("kernel_shape", [3])]), W.node("Slice", ["c", "b", "e", "ax"], ["out"])]
    blob = W.model("c1d", nodes, [W.tensor("K", K), i64("b", [4]), i64("e", [5]), i64("ax", [1])], [W.value_info("X", ["N", C, L])],
                   [W.value_info("out", ["N", 1, L - 2])])
    x = _x(37, C, L, seed=17)
    ref = torch.nn.functional.conv1d(torch.from_numpy(x).double(), torch.from_numpy(K).double()).numpy()[:, 4]
    p = W.write(str(tmp_path / "c1d.onnx"), blob)
    api.load_model("c1d", p)
    try:
        got = np.stack([api.predict_from_blob("c1d", x[i].tobytes()).reshape(-1) for i in range(37)])
    finally:
        api.unload_model("c1d")
    assert worst_ratio(got, ref) <= 1.0


def test_nan_poisons_its_own_row_only(api, tmp_path):
    spec = W.recurrent_spec("GRU", T=8, F=4, H=20, direction="bidirectional")
    x = _x(40, 8, 4, seed=6)
    blob = _model(spec)
    clean = _predict(api, tmp_path, blob, x)
    x2 = x.copy()
    x2[13, 2, 1] = np.nan
    got = _predict(api, tmp_path, blob, x2)
    clean, got = clean.reshape(40, -1), got.reshape(40, -1)
    keep = np.arange(40) != 13
    assert np.array_equal(got[keep], clean[keep]) and np.isnan(got[13]).any()


def test_sql_surfaces(api, tmp_path):
    from infera_amd import sqlharness

    T, F, H, rows = 6, 4, 16, 2048  # (one DataChunk)
    rng = np.random.default_rng(12)
    spec = W.recurrent_spec("LSTM", T=T, F=F, H=H)
    Wd, bd = rng.normal(0, 0.3, (H, 1)).astype(np.float32), np.zeros(1, np.float32)
    p = W.write(str(tmp_path / "sql.onnx"), W.recurrent_from_spec(spec, flat=True, tail="last_gather", head=(Wd, bd, "Sigmoid")))
    x = _x(rows, T, F, seed=13).reshape(rows, T * F)
    api.load_model("direct", p)
    try:
        ref = api.predict("direct", x)
    finally:
        api.unload_model("direct")
    sqlharness.sql("infera_load_model", "rnn_sql", p)
    try:
        got = sqlharness.sql("infera_predict", "rnn_sql", *[np.ascontiguousarray(x[:, j]) for j in range(T * F)])
        assert np.array_equal(np.asarray(got, np.float32).reshape(-1), ref.reshape(-1))
    finally:
        sqlharness.sql("infera_unload_model", "rnn_sql")
    # a vector per row through infera_predict_multi_list: the final state Y_h [N, H] of a GRU
    pv = W.write(str(tmp_path / "sql_vec.onnx"), W.recurrent_from_spec(W.recurrent_spec("GRU", T=T, F=F, H=H), flat=True, tail="y_h"))
    api.load_model("direct_vec", pv)
    try:
        ref = api.predict("direct_vec", x)
    finally:
        api.unload_model("direct_vec")
    assert ref.shape == (rows, H)
    sqlharness.sql("infera_load_model", "rnn_vec", pv)
    try:
        got = sqlharness.sql("infera_predict_multi_list", "rnn_vec", *[np.ascontiguousarray(x[:, j]) for j in range(T * F)])
        assert np.array_equal(np.stack(got), ref)
    finally:
        sqlharness.sql("infera_unload_model", "rnn_vec")
