"""Statically quantised ONNX models on the GPU: every QDense result against the integer definition BIT FOR BIT, the
two spellings and the two buffer forms against each other, the float fallback against the float references."""
from __future__ import annotations

import itertools
import threading

import numpy as np
import pytest

from infera_amd import onnx_writer as W
from infera_amd import synth

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 1e-6


@pytest.fixture(scope="module")
def api(built):
    from infera_amd import capi

    assert capi.device_count() >= 1, capi.get_devices()
    return capi


def _predict(api, tmp_path, blob, x, name="q"):
    p = W.write(str(tmp_path / f"{name}.onnx"), blob)
    api.load_model(name, p)
    try:
        return api.predict(name, np.ascontiguousarray(x, dtype=np.float32))
    finally:
        api.unload_model(name)


def same_bits(got, want):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    return got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def layer_input(spec, rows, seed):
    """Rows that cover the input quantisation's whole range and a little beyond it at both ends."""
    s, z = float(spec["q"][0][0]), spec["q"][0][1]
    lo, hi = W._qrange(spec["x_type"])
    u = synth.table(seed, 0, rows, spec["dims"][0]).astype(np.float64)  # [-1, 1)
    mid, half = ((lo + hi) / 2 - z) * s, (hi - lo) / 2 * s
    return (mid + 1.1 * half * u).astype(np.float32)


WEIGHTS = {"int8_symmetric": dict(w_type="int8", per_channel=False), "int8_per_channel": dict(w_type="int8", per_channel=True),
           "uint8_per_channel_zero_points": dict(w_type="uint8", per_channel=True, w_zero_points=True)}
X_FORMS = [("uint8", 0), ("uint8", 128), ("uint8", 3), ("int8", 0), ("int8", -5)]
BIASES = ["int32", "f32", None]
ACTS = ["Relu", ("Clip", -0.3, 0.4), ""]
SHAPES = [(1, 1), (5, 3), (30, 31), (33, 32), (64, 33), (100, 100), (561, 256), (30, 256), (561, 1), (64, 3), (1, 100), (100, 31)]
ROWS = [1, 31, 33, 301]


def _single_case(api, tmp_path, K, M, rows, x_form, wname, bias, act, seed):
    spec = W.quantized_mlp_spec((K, M), acts=[act], x_type=x_form[0], x_zero_point=x_form[1], bias=bias, seed=seed, **WEIGHTS[wname])
    x = layer_input(spec, rows, seed + 1)
    got = _predict(api, tmp_path, W.quantized_from_spec(spec, layer=("matmul_add", "gemm", "gemm_transb")[seed % 3]), x)
    want = W.quantized_reference(spec, x, "int")
    assert same_bits(got, want), (K, M, rows, x_form, wname, bias, act, int((got != want).sum()), float(np.abs(got - want).max() / spec["q"][1][0]))


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=lambda i: "K%d_M%d" % SHAPES[i])
def test_single_layer_shapes_bit_for_bit(api, tmp_path, i):
    K, M = SHAPES[i]
    forms = list(itertools.product(X_FORMS, WEIGHTS, BIASES, ACTS))
    for j, rows in enumerate(ROWS):  # every shape at every row count, walking through the forms
        x_form, wname, bias, act = forms[(17 * i + 5 * j) % len(forms)]
        _single_case(api, tmp_path, K, M, rows, x_form, wname, bias, act, seed=100 + 4 * i + j)


@pytest.mark.parametrize("x_form", X_FORMS, ids=lambda f: "%s_zp%d" % f)
def test_single_layer_every_form_bit_for_bit(api, tmp_path, x_form):
    for j, (wname, bias, act) in enumerate(itertools.product(WEIGHTS, BIASES, ACTS)):
        _single_case(api, tmp_path, 33, 33, 33, x_form, wname, bias, act, seed=300 + j)


def hand_spec(wq, w_scale, w_zp, qx, qy, x_type="int8", w_type="int8", act=""):
    K, M = wq.shape
    layer = {"wq": wq.astype(np.int64), "w_scale": np.asarray(w_scale, np.float32).reshape(-1), "w_zp": np.asarray(w_zp, np.int64).reshape(-1), "bias_q": None,
             "bias_f": None}
    return {"dims": [K, M], "acts": [act], "x_type": x_type, "w_type": w_type, "per_channel": layer["w_scale"].size > 1, "layers": [layer],
            "q": [(np.float32(qx[0]), qx[1]), (np.float32(qy[0]), qy[1])], "tail": ""}


def test_layout_with_an_asymmetric_matrix(api, tmp_path):
    K, M = 70, 37
    k, m = np.meshgrid(np.arange(K), np.arange(M), indexing="ij")
    wq = (7 * k + 13 * m) % 255 - 127
    spec = hand_spec(wq, [1.0], [0], (1.0, 0), (1.0, 0))
    rows = 2 * K + 3
    x = np.zeros((rows, K), np.float32)
    x[np.arange(rows), np.arange(rows) % K] = 1.0  # one-hot: each output element is one weight
    got = _predict(api, tmp_path, W.quantized_from_spec(spec), x)
    assert np.array_equal(got, wq[np.arange(rows) % K].astype(np.float32))
    assert same_bits(got, W.quantized_reference(spec, x, "int"))


def test_rounding_and_saturation(api, tmp_path):
    K = 32
    spec = hand_spec(np.eye(K, dtype=np.int64), [4.0], [0], (0.25, 0), (1.0, 0))  # mult = 1: the result IS the quantised input
    halves = (np.arange(-12, 12) + 0.5) * 0.25  # x / scale = k + 0.5 for even and odd k
    far = np.array([1e4, -1e4, 1e30, -1e30, np.inf, -np.inf, 31.75, -32.0], np.float64)
    x = np.concatenate([halves, far]).astype(np.float32)[:, None] * np.ones((1, K), np.float32)
    got = _predict(api, tmp_path, W.quantized_from_spec(spec), x)
    want = np.concatenate([np.rint(np.arange(-12, 12) + 0.5), [127, -128, 127, -128, 127, -128, 127, -128]]).astype(np.float32)
    assert np.array_equal(got, want[:, None] * np.ones((1, K), np.float32))
    assert same_bits(got, W.quantized_reference(spec, x, "int"))


def test_accumulator_at_the_cap(api, tmp_path):
    K, M, rows = (2 ** 31 - 1) // (255 * 255), 3, 17
    # 255 against -255 in every term: acc = -K * 255 * 255, the most negative sum the cap admits
    spec = hand_spec(np.full((K, M), -128), [2.0 ** -25], [127], (1.0, 0), (1.0, 0), x_type="uint8")
    x = np.full((rows, K), 1e9, np.float32)
    want = W.quantized_reference(spec, x, "int")
    got = _predict(api, tmp_path, W.quantized_from_spec(spec), x)
    assert same_bits(got, want) and float(want[0, 0]) == 0.0  # (uint8 result: the negative sum saturates at the zero point)
    spec = hand_spec(np.full((K, M), -128), [2.0 ** -25], [127], (1.0, 0), (1.0, 0), x_type="uint8")
    spec["q"][1] = (np.float32(1.0), 128)
    want = W.quantized_reference(spec, x, "int")
    assert float(want[0, 0]) == float(np.rint(np.float32(-K * 255 * 255) * np.float32(2.0 ** -25)))
    assert same_bits(_predict(api, tmp_path, W.quantized_from_spec(spec), x), want)


# ---- whole networks ---------------------------------------------------------------------------------------------------------------------

def one_step_cap(got, ref, step):
    d = np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64)) / step
    return float((d > 1e-3).mean()) <= 1e-3 and float(d.max()) <= 1.0 + 1e-3


def test_mlp_bit_for_bit_and_call_paths(api, tmp_path, monkeypatch):
    dims, rows = (128, 256, 64, 1), 301
    spec = W.quantized_mlp_spec(dims, seed=1234)
    x = synth.table(1334, 0, rows, dims[0])
    want = W.quantized_reference(spec, x, "int")
    p = W.write(str(tmp_path / "net.onnx"), W.quantized_from_spec(spec))
    api.load_model("net", p)
    monkeypatch.setenv("INFERA_QDENSE_BYTES", "0")
    api.load_model("net_f32", p)
    monkeypatch.delenv("INFERA_QDENSE_BYTES")
    try:
        assert [q["out_bytes"] for q in api.get_plan("net")["qdense"]] == [True, True, False]
        assert not any(q["out_bytes"] or q["in_bytes"] for q in api.get_plan("net_f32")["qdense"])
        ref = api.predict("net", x)
        assert same_bits(ref, want)
        assert same_bits(api.predict("net_f32", x), ref)  # byte buffers == f32 buffers
        assert one_step_cap(ref, W.quantized_reference(spec, x, "f64"), float(spec["q"][-1][0]))
        for n in (1, 31, 33):
            assert same_bits(api.predict("net", np.ascontiguousarray(x[:n])), ref[:n]), n
        assert same_bits(api.predict("net", np.ascontiguousarray(x[100:117])), ref[100:117])
        assert same_bits(api.predict_columns("net", [np.ascontiguousarray(x[:, j]) for j in range(dims[0])]), ref)
        api.register_host_memory(x)
        try:
            assert same_bits(api.predict("net", x), ref)
        finally:
            api.unregister_host_memory(x)
        assert same_bits(api.predict_from_blob("net", x[5].tobytes()).reshape(-1), ref[5])
        dev = api.device_ordinal(0)
        d_in, d_out = api.DeviceBuffer(dev, x.nbytes), api.DeviceBuffer(dev, ref.nbytes)
        d_in.upload(x)
        api.predict_device("net", d_in, rows, dims[0], d_out)
        assert same_bits(d_out.download(ref.shape), ref)
        api.load_model("net_sel", p + "#Y")  # the output selected by name
        try:
            assert same_bits(api.predict("net_sel", x), ref)
        finally:
            api.unload_model("net_sel")
        outs, errs = [None] * 8, []

        def call(i):
            try:
                outs[i] = api.predict("net", x[: 100 + 25 * i])
            except Exception as e:  # noqa: BLE001
                errs.append(e)

        ts = [threading.Thread(target=call, args=(i,)) for i in range(8)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not errs, errs
        assert all(same_bits(outs[i], ref[: 100 + 25 * i]) for i in range(8))
    finally:
        api.unload_model("net")
        api.unload_model("net_f32")


@pytest.mark.parametrize("dims,tail,seed", [((128, 256, 64, 1), "", 1234), ((30, 100, 2), "Softmax", 77)])
def test_qdq_and_qlinear_spellings_give_the_same_bits(api, tmp_path, monkeypatch, dims, tail, seed):
    spec = W.quantized_mlp_spec(dims, seed=seed, bias=None, tail=tail)
    x = synth.table(seed + 100, 0, 301, dims[0])
    qdq = _predict(api, tmp_path, W.quantized_from_spec(spec, "qdq"), x, "qdq")
    assert same_bits(_predict(api, tmp_path, W.quantized_from_spec(spec, "qlinear"), x, "qlin"), qdq)
    monkeypatch.setenv("INFERA_QDENSE_BYTES", "0")
    assert same_bits(_predict(api, tmp_path, W.quantized_from_spec(spec, "qlinear"), x, "qlin32"), qdq)
    monkeypatch.delenv("INFERA_QDENSE_BYTES")
    if not tail:
        assert same_bits(qdq, W.quantized_reference(spec, x, "int"))
    else:  # the integer layers are exact; the Softmax behind them meets the usual bar
        want = W.quantized_reference(spec, x, "int").astype(np.float64)
        assert float(np.max(np.abs(qdq - want) / (RTOL * np.abs(want) + ATOL))) <= 1.0
    assert one_step_cap(W.quantized_reference(spec, x, "int", tail=False), W.quantized_reference(spec, x, "f64", tail=False), float(spec["q"][-1][0]))


def test_softmax_network_with_bias(api, tmp_path):
    spec = W.quantized_mlp_spec((30, 100, 2), seed=77, tail="Softmax")
    x = synth.table(177, 0, 301, 30)
    got = _predict(api, tmp_path, W.quantized_from_spec(spec, layer="gemm"), x)
    want = W.quantized_reference(spec, x, "int").astype(np.float64)
    assert float(np.max(np.abs(got - want) / (RTOL * np.abs(want) + ATOL))) <= 1.0


def test_window_input(api, tmp_path):
    """[rows, T, K] through QLinearMatMul and through the QDQ MatMul: the layer runs on each of the rows * T vectors."""
    T, K, M, rows = 5, 33, 20, 31
    spec = W.quantized_mlp_spec((K, M), acts=[""], bias=None, seed=9)
    x = layer_input(spec, rows * T, 10)
    want = W.quantized_reference(spec, x, "int")
    for form in ("qlinear", "qdq"):
        got = _predict(api, tmp_path, W.quantized_from_spec(spec, form, window=T), x.reshape(rows, T * K), form)
        assert same_bits(got.reshape(rows * T, M), want), form


# ---- the float fallback -------------------------------------------------------------------------------------------------------------------

def test_fake_quant_around_a_sigmoid(api, tmp_path):
    cols, s, z = 12, np.float32(0.02), 3
    inits = [W.tensor("s", np.array(s, np.float32)), W.tensor("z", np.array(z, np.uint8))]
    nodes = [W.node("QuantizeLinear", ["X", "s", "z"], ["Xq"]), W.node("DequantizeLinear", ["Xq", "s", "z"], ["Xd"]), W.node("Sigmoid", ["Xd"], ["H"]),
             W.node("QuantizeLinear", ["H", "s", "z"], ["Hq"]), W.node("DequantizeLinear", ["Hq", "s", "z"], ["Y"])]
    blob = W.model("fq", nodes, inits, [W.value_info("X", ["N", cols])], [W.value_info("Y", ["N", cols])])
    x = (synth.table(4, 0, 301, cols) * 4.0).astype(np.float32)
    x[0, :4] = [np.inf, -np.inf, 1e30, -1e30]
    got = _predict(api, tmp_path, blob, x)

    def fq(v):
        with np.errstate(over="ignore"):
            return ((np.clip(np.rint(v / s) + np.float32(z), 0, 255) - np.float32(z)) * s).astype(np.float32)
    h = fq(x)
    want = fq((1.0 / (1.0 + np.exp(-h.astype(np.float64)))).astype(np.float32))
    assert one_step_cap(got, want, float(s))
    # the input side alone is exact: the values the Sigmoid reads
    assert same_bits(_predict(api, tmp_path, W.model("fq1", nodes[:2], inits, [W.value_info("X", ["N", cols])], [W.value_info("Xd", ["N", cols])]), x, "fq1"), h)


def test_weight_only_model_meets_the_usual_bar(api, tmp_path):
    spec = W.quantized_mlp_spec((30, 100, 2), seed=77, tail="Softmax")
    x = synth.table(177, 0, 301, 30)
    got = _predict(api, tmp_path, W.quantized_from_spec(spec, weight_only=True), x)
    want = W.quantized_reference(spec, x, "f64", weight_only=True).astype(np.float64)
    assert float(np.max(np.abs(got - want) / (RTOL * np.abs(want) + ATOL))) <= 1.0
