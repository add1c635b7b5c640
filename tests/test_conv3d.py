"""Conv, MaxPool and AveragePool on [N, C, D, H, W] without a GPU (INTEGRATION.md 2.6 "3-D convolutions"): the plan of an R3D block model, the
shape and work of one strided, padded, dilated layer, and what is refused at load, by node name."""
from __future__ import annotations

import numpy as np
import pytest

from infera_amd import onnx_writer as W


@pytest.fixture(scope="module")
def api(built):
    from infera_amd import capi

    return capi


def load_plan(api, tmp_path, blob, name="c3d"):
    api.load_model(name, W.write(str(tmp_path / f"{name}.onnx"), blob))
    try:
        return api.get_plan(name)
    finally:
        api.unload_model(name)


def test_r3d_block_model_plan(api, tmp_path):
    blob, ops = W.r3d_net()
    plan = load_plan(api, tmp_path, blob)
    steps = plan["plan"]["steps"]
    assert [s["kind"] for s in steps] == ["Conv3d", "Pool3d", "Conv3d", "Conv3d", "BinaryAct", "Conv3d", "Conv3d", "Conv3d", "BinaryAct", "GlobalAvgPool", "Dense"]
    convs = [s for s in steps if s["kind"] == "Conv3d"]
    assert len(convs) == sum(o[0] == "conv" for o in ops) and all("+BatchNormalization" in s["origin"] and s["bias"] for s in convs)
    assert [s.get("act", "") for s in convs] == ["Relu", "Relu", "", "Relu", "", ""]  # (the block's second Relu follows the Add)
    assert all(s["exec"] == "conv3d_mfma" and s["input_window"] == "global" and s["lds_bytes"] == 0 for s in convs)  # (staging is opt-in: INFERA_CONV3D_STAGE=1)
    assert plan["activation_layout"] == "NCHW" and plan["plan"]["output_shape"] == [-1, 3]


def test_one_layer_shape_and_flops(api, tmp_path):
    """out = floor((in + pads - dilation (k - 1) - 1) / stride) + 1 per axis; K = (C / g) kd kh kw; flops = 2 K M OD OH OW"""
    w = np.zeros((6, 4, 2, 3, 2), np.float32)
    plan = load_plan(api, tmp_path, W.conv3d_layer(w, None, (5, 6, 7), strides=[2, 1, 1], pads=[0, 1, 2, 1, 0, 2], dilations=[2, 1, 2]))
    s = plan["plan"]["steps"][0]
    assert (s["in_dhw"], s["out_dhw"], s["k"], s["K"], s["M"], s["groups"]) == ([5, 6, 7], [2, 5, 9], [2, 3, 2], 48, 6, 1)
    assert (s["strides"], s["pads"], s["dilations"]) == ([2, 1, 1], [0, 1, 2, 1, 0, 2], [2, 1, 2])
    assert plan["plan"]["output_shape"] == [-1, 6, 2, 5, 9] and plan["plan"]["flops_per_row"] == 2 * 48 * 6 * 2 * 5 * 9
    grouped = load_plan(api, tmp_path, W.conv3d_layer(np.zeros((8, 1, 3, 3, 3), np.float32), None, (3, 5, 5), group=8, auto_pad="SAME_UPPER"))
    assert (grouped["plan"]["steps"][0]["exec"], grouped["plan"]["steps"][0]["out_dhw"]) == ("conv3d_generic", [3, 5, 5])


def _two_nodes(first, second, inits, c=2, elem=W.FLOAT):
    return W.model("refused", [first, second], inits, [W.value_info("X", ["N", c, 3, 4, 4], elem)], [W.value_info("Y", ["N", "c", "d", "h", "w"], elem)], opset=17)


def _qdq():
    wq = W.node("DequantizeLinear", ["wq", "ws", "wz"], ["w"], name="dq")
    inits = [W.tensor("wq", np.ones((2, 2, 1, 1, 1), np.int8)), W.tensor("ws", np.array(0.5, np.float32)), W.tensor("wz", np.array(0, np.int8))]
    return _two_nodes(wq, W.node("Conv", ["X", "w"], ["Y"], name="qconv"), inits)


W3 = np.zeros((2, 2, 1, 1, 1), np.float32)
REFUSED = [
    ("non-constant weights", lambda: _two_nodes(W.node("Relu", ["X"], ["w"]), W.node("Conv", ["X", "w"], ["Y"], name="cv"), []), "node 'cv' (Conv): unsupported operator form: the weights"),
    ("kernel rank", lambda: W.conv3d_layer(W3[..., 0], None, (3, 4, 4)), "does not have the rank of the input"),
    ("bias length", lambda: W.conv3d_layer(W3, np.zeros(3, np.float32), (3, 4, 4)), "the bias has 3 entries for M = 2"),
    ("Pad in front", lambda: _two_nodes(W.node("Pad", ["X", "p"], ["xp"], name="pad"), W.node("Conv", ["xp", "w"], ["Y"]), [W.tensor("p", np.array([0, 0, 1, 1, 1, 0, 0, 1, 1, 1], np.int64)), W.tensor("w", W3)]),
     "node 'pad' (Pad): unsupported operator form: its data is [-1,2,3,4,4]"),  # (the refusal every Pad outside [N,C,H,W] and STFT signals gets)
    ("QDQ", _qdq, "node 'qconv' (Conv): unsupported operator form: a quantised"),
    ("float16", lambda: W.conv3d_layer(W3.astype(np.float16), None, (3, 4, 4), elem=W.FLOAT16), "unsupported operator form: a float16 convolution"),
    ("kernel extent", lambda: W.conv3d_layer(np.zeros((1, 1, 1, 1, 65), np.float32), None, (1, 1, 80)), "a kernel extent above 64"),
    ("2^31 per image", lambda: W.conv3d_layer(np.zeros((1, 2, 1, 1, 1), np.float32), None, (1024, 1024, 1024)), "2^31 or more per image"),
    ("pads length", lambda: W.conv3d_layer(W3, None, (3, 4, 4), pads=[1, 1, 1, 1]), "pads must have 6 entries"),
    ("zero stride", lambda: W.conv3d_layer(W3, None, (3, 4, 4), strides=[1, 0, 1]), "strides must be >= 1"),
    ("empty output", lambda: W.conv3d_layer(np.zeros((2, 2, 4, 1, 1), np.float32), None, (3, 4, 4)), "empty spatial output"),
    ("groups", lambda: W.conv3d_layer(W3, None, (3, 4, 4), group=3), "channel/group mismatch"),
    ("pool kernel_shape", lambda: W.pool3d_layer("MaxPool", 2, (3, 4, 4), kernel_shape=[2, 2]), "kernel_shape must have 3 entries"),
    ("ConvTranspose", lambda: _two_nodes(W.node("Identity", ["X"], ["x"]), W.node("ConvTranspose", ["x", "w"], ["Y"], name="ct"), [W.tensor("w", W3)]), "rank 3 or 4"),
]


@pytest.mark.parametrize("build,fragment", [r[1:] for r in REFUSED], ids=[r[0] for r in REFUSED])
def test_refused_at_load_by_name(api, tmp_path, build, fragment):
    with pytest.raises(api.InferaError) as e:
        load_plan(api, tmp_path, build(), "c3d_refused")
    assert fragment in str(e.value) and "only [N,C,L] / [N,C,H,W] activations" not in str(e.value), str(e.value)
