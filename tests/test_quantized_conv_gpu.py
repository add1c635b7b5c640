"""Statically quantised convolutions on the GPU: every QConv2d result against the integer definition BIT FOR BIT -- in
NCHW and in channel-quad planes, with the input window staged in LDS and read from global memory --, the two spellings against each
other, and the grouped float fallback against the float reference."""
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


def _run(api, tmp_path, blob, x, name="qc", plan=False):
    p = W.write(str(tmp_path / f"{name}.onnx"), blob)
    api.load_model(name, p)
    try:
        got = _images(api, name, x)
        return (got, api.get_plan(name)) if plan else got
    finally:
        api.unload_model(name)


def _images(api, name, x):
    """[N, ...] images through infera_predict_from_blob (the entry that takes tensors of any rank)"""
    return api.predict_from_blob(name, np.ascontiguousarray(x, dtype=np.float32).tobytes())


def same_bits(got, want):
    got, want = np.ascontiguousarray(got, np.float32).reshape(-1), np.ascontiguousarray(want, np.float32).reshape(-1)
    return got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def layer_input(spec, rows, seed):
    """Images that cover the input quantisation's whole range and a little beyond it at both ends."""
    s, z = float(spec["q"]["X"][0]), spec["q"]["X"][1]
    lo, hi = W._qrange(spec["x_type"])
    n = int(np.prod(spec["in_shape"]))
    u = synth.table(seed, 0, rows, n).astype(np.float64)  # [-1, 1)
    mid, half = ((lo + hi) / 2 - z) * s, (hi - lo) / 2 * s
    return (mid + 1.1 * half * u).astype(np.float32).reshape([rows] + list(spec["in_shape"]))


WEIGHTS = {"int8_symmetric": dict(w_type="int8", per_channel=False), "int8_per_channel": dict(w_type="int8", per_channel=True),
           "uint8_per_channel_zero_points": dict(w_type="uint8", per_channel=True, w_zero_points=True)}
X_FORMS = [("uint8", 0), ("uint8", 128), ("uint8", 3), ("int8", 0), ("int8", -5)]
BIASES = ["int32", "f32", None]
ACTS = ["Relu", ("Clip", -0.3, 0.4), ""]
FORMS = list(itertools.product(X_FORMS, WEIGHTS, BIASES, ACTS))
# (kernel, stride, pads (top, left, bottom, right), dilation); "conv1d": [N, C, L] input
GEOMETRIES = {"1x1": dict(k=1), "3x3_pad1": dict(k=3, pads=1), "7x7_stride2_pad3": dict(k=7, stride=2, pads=3), "3x3_dilation2": dict(k=3, dilation=2),
              "3x3_pads_0_1_2_1": dict(k=3, pads=(0, 1, 2, 1)), "conv1d": dict(k=3, pads=1)}
CHANNELS, FEATURES, IMAGES, ROWS = [1, 3, 4, 17, 64], [1, 4, 17, 33], [(5, 7), (9, 9)], [1, 3, 17]


def _layer_case(api, tmp_path, geom, C, M, hw, rows, form, seed, pooled=False):
    x_form, wname, bias, act = form
    in_shape = (C, hw[0] * hw[1]) if geom == "conv1d" else (C,) + tuple(hw)
    spec = W.quantized_conv_spec("layer", in_shape, m=M, act=act, bias=bias, x_type=x_form[0], x_zero_point=x_form[1], seed=seed, pooled=pooled,
                                 **GEOMETRIES[geom], **WEIGHTS[wname])
    x = layer_input(spec, rows, seed + 1)
    got, plan = _run(api, tmp_path, W.quantized_conv_from_spec(spec), x, plan=True)
    assert [s["kind"] for s in plan["plan"]["steps"]][0] == "QConv2d"
    assert plan["activation_layout"] == ("NC/4HW4" if pooled else "NCHW"), plan["activation_layout"]
    want = W.quantized_conv_reference(spec, x, "int")
    step = float(spec["q"]["C0"][0])
    assert same_bits(got, want), (geom, C, M, hw, rows, form, int((got.reshape(-1) != want.reshape(-1)).sum()), float(np.abs(got.reshape(-1) - want.reshape(-1)).max() / step))


@pytest.mark.parametrize("geom", list(GEOMETRIES))
def test_single_layers_in_nchw_bit_for_bit(api, tmp_path, geom):
    g = list(GEOMETRIES).index(geom)
    for j, (C, M) in enumerate(itertools.product(CHANNELS, FEATURES)):  # every (C, M) at every geometry, walking through the forms, images and rows
        _layer_case(api, tmp_path, geom, C, M, IMAGES[(j + g) % 2], ROWS[(j + g) % 3], FORMS[(17 * g + 7 * j) % len(FORMS)], seed=500 + 20 * g + j)


@pytest.mark.parametrize("x_form", X_FORMS, ids=lambda f: "%s_zp%d" % f)
def test_single_layer_every_form_bit_for_bit(api, tmp_path, x_form):
    for j, (wname, bias, act) in enumerate(itertools.product(WEIGHTS, BIASES, ACTS)):
        _layer_case(api, tmp_path, "3x3_pad1", 17, 17, (5, 7), 3, (x_form, wname, bias, act), seed=700 + j)


@pytest.mark.parametrize("geom", list(GEOMETRIES))
def test_single_layers_in_channel_quads_bit_for_bit(api, tmp_path, geom):
    g = list(GEOMETRIES).index(geom)
    for j, (C, M) in enumerate(itertools.product([4, 64], [4, 36])):
        _layer_case(api, tmp_path, geom, C, M, IMAGES[(j + g) % 2], ROWS[(j + g) % 3], FORMS[(11 * g + 5 * j) % len(FORMS)], seed=800 + 10 * g + j, pooled=True)


def test_window_from_global_memory_gives_the_same_bits(api, tmp_path, monkeypatch):
    """INFERA_QCONV_STAGE=0: the variant that serves footprints beyond the LDS budget, on shapes the staged one serves too."""
    monkeypatch.setenv("INFERA_QCONV_STAGE", "0")
    for j, geom in enumerate(GEOMETRIES):
        _layer_case(api, tmp_path, geom, 17, 33, IMAGES[j % 2], 3, FORMS[(13 * j) % len(FORMS)], seed=900 + j)
        _layer_case(api, tmp_path, geom, 4, 36, IMAGES[j % 2], 17, FORMS[(13 * j + 1) % len(FORMS)], seed=920 + j, pooled=True)


def hand_spec(wq, w_scale, w_zp, qx, qy, hw, x_type="int8", w_type="int8", pads=(0, 0, 0, 0), bias_q=None, act=""):
    M, C = wq.shape[:2]
    w_scale = np.asarray(w_scale, np.float32).reshape(-1)
    op = {"op": "conv", "in": "X", "out": "C0", "wq": wq.astype(np.int64), "w_scale": w_scale, "w_zp": np.asarray(w_zp, np.int64).reshape(-1), "strides": (1, 1),
          "pads": tuple(pads), "dilations": (1, 1), "group": 1, "act": act, "bias_q": None, "bias_f": None}
    if bias_q is not None:
        op["bias_q"], op["bias_scale"] = np.asarray(bias_q, np.int64), (np.float32(qx[0]) * w_scale).astype(np.float32)
    oh, ow = hw[0] + pads[0] + pads[2] - wq.shape[2] + 1, hw[1] + pads[1] + pads[3] - wq.shape[3] + 1
    return {"name": "hand", "x_type": x_type, "w_type": w_type, "per_channel": w_scale.size > 1, "in_shape": [C, hw[0], hw[1]], "out_shape": [M, oh, ow], "ops": [op],
            "q": {"X": (np.float32(qx[0]), qx[1]), "C0": (np.float32(qy[0]), qy[1])}, "out": "C0"}


def test_delta_image_reads_one_weight_per_output_element(api, tmp_path):
    C, M = 5, 37
    m, k = np.meshgrid(np.arange(M), np.arange(C * 9), indexing="ij")
    wq = ((7 * k + 13 * m) % 255 - 127).reshape(M, C, 3, 3)
    spec = hand_spec(wq, [1.0], [0], (1.0, 3), (1.0, 0), (3, 3), x_type="uint8", pads=(1, 1, 1, 1))
    x = np.zeros((C, C, 3, 3), np.float32)
    x[np.arange(C), np.arange(C), 1, 1] = 1.0  # image r: the quantised value x_zp + 1 at the centre of channel r, x_zp elsewhere
    got = _run(api, tmp_path, W.quantized_conv_from_spec(spec), x).reshape(C, M, 3, 3)
    # output pixel (oh, ow) sees the centre under tap (2 - oh, 2 - ow); uint8 result with zero point 0: negative weights saturate at 0
    want = np.maximum(np.stack([wq[:, r, ::-1, ::-1] for r in range(C)]), 0).astype(np.float32)
    assert np.array_equal(got, want)
    assert same_bits(got, W.quantized_conv_reference(spec, x, "int"))
    spec["q"]["C0"] = (np.float32(1.0), 128)  # ... and with the zero point in the middle every weight comes back (127 -> saturates at 127)
    got = _run(api, tmp_path, W.quantized_conv_from_spec(spec), x).reshape(C, M, 3, 3)
    assert np.array_equal(got, np.stack([wq[:, r, ::-1, ::-1] for r in range(C)]).astype(np.float32))


@pytest.mark.parametrize("x_type,x_zp", [("uint8", 128), ("int8", -5)])
def test_padding_is_the_zero_point(api, tmp_path, x_type, x_zp):
    """A constant image at real 0 through a 3x3 / pad 1 layer: every output, corners included, is the bias term alone."""
    for wname in WEIGHTS:
        spec = W.quantized_conv_spec("layer", (5, 5, 7), m=6, k=3, pads=1, act="", x_type=x_type, x_zero_point=x_zp, seed=31, **WEIGHTS[wname])
        x = np.zeros((3, 5, 5, 7), np.float32)
        got = _run(api, tmp_path, W.quantized_conv_from_spec(spec), x).reshape(3, 6, 5, 7)
        assert same_bits(got, W.quantized_conv_reference(spec, x, "int")), wname
        assert np.array_equal(got, np.broadcast_to(got[:1, :, 2:3, 3:4], got.shape)), wname  # borders == interior, per channel
        assert len(np.unique(got[0, :, 0, 0])) > 1  # (the bias term differs between channels: not all zeros)


def test_accumulator_at_the_cap(api, tmp_path):
    C, M, rows = 1321, 3, 17  # K = 1321 * 25 = 33025 = (2^31 - 1) // (255 * 255)
    assert C * 25 == (2 ** 31 - 1) // (255 * 255)
    spec = hand_spec(np.full((M, C, 5, 5), -128), [2.0 ** -25], [127], (1.0, 0), (1.0, 128), (5, 5), x_type="uint8")
    x = np.full((rows, C, 5, 5), 1e9, np.float32)
    want = W.quantized_conv_reference(spec, x, "int")
    assert float(want.reshape(-1)[0]) == float(np.rint(np.float32(-C * 25 * 255 * 255) * np.float32(2.0 ** -25)))
    assert same_bits(_run(api, tmp_path, W.quantized_conv_from_spec(spec), x), want)


# ---- whole networks ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def resnet():
    spec = W.quantized_conv_spec("resnet", (3, 32, 32), width=8, seed=77)
    x = synth.table(177, 0, 19, 3 * 32 * 32).reshape(19, 3, 32, 32)
    return spec, x, W.quantized_conv_reference(spec, x, "int")


def test_residual_net_both_spellings_bit_for_bit(api, tmp_path, resnet):
    spec, x, want = resnet
    outs = {}
    for form in ("qdq", "qlinear"):
        p = W.write(str(tmp_path / f"{form}.onnx"), W.quantized_conv_from_spec(spec, form))
        api.load_model(form, p)
        try:
            plan = api.get_plan(form)
            assert plan["activation_layout"] == "NC/4HW4" and "Conv2d" not in [s["kind"] for s in plan["plan"]["steps"]]
            assert [q["in_layout"] for q in plan["qconv"]] == ["NCHW"] + ["NC/4HW4"] * 5
            outs[form] = _images(api, form, x)
            assert same_bits(_images(api, form, x[:1]), want[:1]), form
        finally:
            api.unload_model(form)
        assert same_bits(outs[form], want), (form, int((outs[form].reshape(-1) != want.reshape(-1)).sum()))
    assert same_bits(outs["qdq"], outs["qlinear"])


def test_residual_net_from_two_threads(api, tmp_path, resnet):
    spec, x, want = resnet
    p = W.write(str(tmp_path / "net.onnx"), W.quantized_conv_from_spec(spec))
    api.load_model("net2t", p)
    try:
        outs, errs = [None, None], []

        def call(i):
            try:
                outs[i] = _images(api, "net2t", x)
            except Exception as e:  # noqa: BLE001
                errs.append(e)

        ts = [threading.Thread(target=call, args=(i,)) for i in range(2)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not errs, errs
        assert same_bits(outs[0], outs[1]) and same_bits(outs[0], want)
    finally:
        api.unload_model("net2t")


# ---- the float fallback -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("groups", [4, 8], ids=["grouped", "depthwise"])
@pytest.mark.parametrize("form", ["qdq", "qlinear"])
def test_grouped_layers_keep_float_semantics(api, tmp_path, groups, form):
    spec = W.quantized_conv_spec("layer", (8, 9, 9), m=8, k=3, pads=1, groups=groups, act="Relu", seed=41)
    x = layer_input(spec, 17, 42)
    got, plan = _run(api, tmp_path, W.quantized_conv_from_spec(spec, form), x, plan=True)
    assert [s["kind"] for s in plan["plan"]["steps"]] == ["FakeQuant", "Conv2d", "FakeQuant"]
    got = got.reshape(-1).astype(np.float64)
    want = W.quantized_conv_reference(spec, x, "f64").reshape(-1).astype(np.float64)
    step = float(spec["q"]["C0"][0])
    d = np.abs(got - want)
    off = d > RTOL * np.abs(want) + ATOL  # where the float layer's rounding moved a value across a rounding boundary: one step, rarely
    print("share of elements one step off", float(off.mean()), "largest difference in steps", float(d.max() / step))
    assert float(off.mean()) <= 1e-3 and float(d.max()) <= step * (1.0 + 1e-3)
