"""DeformConv at load time, without a GPU (INTEGRATION.md 2.6 "Deformable convolutions"): the plan of a layer and of a DCN block, the layouts and
the kernel the scheduler gives the step, and what is refused, by node name."""
from __future__ import annotations

import numpy as np
import pytest

from infera_amd import onnx_writer as W

CQ, NCHW = "NC/4HW4", "NCHW"


@pytest.fixture(scope="module")
def api(built):
    from infera_amd import capi

    return capi


def load_plan(api, tmp_path, blob, name="dcn"):
    api.load_model(name, W.write(str(tmp_path / f"{name}.onnx"), blob))
    try:
        return api.get_plan(name)
    finally:
        api.unload_model(name)


def w_of(m, c, kh=3, kw=3):
    return np.ones((m, c, kh, kw), np.float32)


def test_the_plan_of_a_layer(api, tmp_path):
    blob = W.deform_conv_layer(w_of(5, 4, 2, 3), np.zeros(5, np.float32), (9, 8), mask=True, act="Relu", strides=[2, 1], pads=[1, 0, 2, 1], dilations=[2, 1], offset_group=2)
    plan = load_plan(api, tmp_path, blob)
    s = [x for x in plan["plan"]["steps"] if x["kind"] == "DeformConv2d"]
    assert len(s) == 1 and [x["kind"] for x in plan["plan"]["steps"]].count("SliceCols") == 3
    want = dict(C=4, M=5, in_hw=[9, 8], out_hw=[5, 7], k=[2, 3], strides=[2, 1], pads=[1, 0, 2, 1], dilations=[2, 1], groups=1, offset_groups=2, mask=True, bias=True, act="Relu")
    assert {k: s[0][k] for k in want} == want
    assert plan["plan"]["flops_per_row"] == 2 * (4 * 6) * 5 * 5 * 7
    # the operands are columns of the call, in the caller's element order
    assert plan["deformconv"] == [dict(step=3, exec="deformconv_mfma", in_layout=NCHW, out_layout=NCHW, offset_layout=NCHW, lds_bytes=8 * 6 * 32 * 4)]


def test_a_block_whose_offsets_are_whole_quads_stays_on_channel_quads(api, tmp_path):
    plan = load_plan(api, tmp_path, W.dcn_block(k=2)[0])  # (8 offset channels, 4 mask channels)
    assert [s["kind"] for s in plan["plan"]["steps"]] == ["Conv2d", "Conv2d", "Conv2d", "DeformConv2d", "Conv2d", "GlobalAvgPool"]
    assert plan["activation_layout"] == CQ
    assert plan["deformconv"] == [dict(step=3, exec="deformconv_mfma", in_layout=CQ, out_layout=CQ, offset_layout=CQ, lds_bytes=8 * 4 * 32 * 4)]
    s = plan["plan"]["steps"][3]
    assert (s["in"], s["in1"], s["in2"], s["act"]) == (plan["plan"]["steps"][0]["out"], plan["plan"]["steps"][1]["out"], plan["plan"]["steps"][2]["out"], "Relu")


def test_a_3x3_block_stays_in_nchw(api, tmp_path):
    plan = load_plan(api, tmp_path, W.dcn_block(k=3)[0])  # (18 offset channels: no whole quads)
    assert plan["activation_layout"] == NCHW
    assert plan["deformconv"] == [dict(step=3, exec="deformconv_mfma", in_layout=NCHW, out_layout=NCHW, offset_layout=NCHW, lds_bytes=8 * 9 * 32 * 4)]


def test_the_generic_kernel_takes_groups_large_kernels_and_the_knob(api, tmp_path, monkeypatch):
    assert load_plan(api, tmp_path, W.deform_conv_layer(w_of(4, 2), None, (5, 5), group=2))["deformconv"][0]["exec"] == "deformconv_generic"
    assert load_plan(api, tmp_path, W.deform_conv_layer(w_of(2, 1, 5, 10), None, (6, 11)))["deformconv"][0]["exec"] == "deformconv_generic"  # (50 taps)
    monkeypatch.setenv("INFERA_DEFORMCONV_MFMA", "0")
    assert load_plan(api, tmp_path, W.deform_conv_layer(w_of(4, 4), None, (5, 5)))["deformconv"][0] == dict(step=2, exec="deformconv_generic", in_layout=NCHW, out_layout=NCHW,
                                                                                                          offset_layout=NCHW, lds_bytes=0)


L = W.deform_conv_layer
REFUSALS = [  # (id, the model, a piece of the reason)
    ("w_not_constant", lambda: L(w_of(4, 4), None, (5, 5), w_input=True), "W must be a constant"),
    ("b_not_constant", lambda: L(w_of(4, 4), np.zeros(4, np.float32), (5, 5), consts=("B",)), "B must be a constant"),
    ("constant_x", lambda: L(w_of(4, 4), None, (5, 5), consts=("X",)), "X is a constant"),
    ("constant_offset", lambda: L(w_of(4, 4), None, (5, 5), consts=("O",)), "offset is a constant"),
    ("rank_3", lambda: L(w_of(4, 4), None, (5, 5), off_dims=[18, 9]), "only rank 4"),
    ("offset_channels", lambda: L(w_of(4, 4), None, (5, 5), off_dims=[9, 3, 3]), "its offset [-1,9,3,3] disagrees"),
    ("offset_extents", lambda: L(w_of(4, 4), None, (5, 5), off_dims=[18, 3, 4]), "its offset [-1,18,3,4] disagrees"),
    ("mask_channels", lambda: L(w_of(4, 4), None, (5, 5), mask=True, mask_dims=[18, 3, 3]), "its mask [-1,18,3,3] disagrees"),
    ("mask_extents", lambda: L(w_of(4, 4), None, (5, 5), mask=True, mask_dims=[9, 5, 5]), "its mask [-1,9,5,5] disagrees"),
    ("offset_group", lambda: L(w_of(4, 4), None, (5, 5), offset_group=3), "offset_group = 3 does not divide C = 4"),
    ("group_c", lambda: L(w_of(4, 2), None, (5, 5), x_dims=[3, 5, 5], group=2), "group = 2 does not divide C = 3"),
    ("group_m", lambda: L(w_of(3, 2), None, (5, 5), group=2), "group = 2 does not divide C = 4 and M = 3"),
    ("symbolic_hw", lambda: L(w_of(4, 4), None, (5, 5), four_d=True, x_dims=[4, "H", "W"]), "symbolic spatial extents"),
    ("kernel_65", lambda: L(w_of(1, 1, 65, 1), None, (65, 1)), "a kernel extent above 64"),
    ("result_2_31", lambda: L(w_of(1 << 16, 1, 1, 1), None, (256, 128)), "2^31"),
    ("float16", lambda: L(w_of(4, 4), None, (5, 5), four_d=True, elem=W.FLOAT16), "float16"),
    ("quantised", lambda: L(w_of(4, 4), None, (5, 5), quantize=True), "quantised tensor"),
    ("strides_length", lambda: L(w_of(4, 4), None, (5, 5), off_dims=[18, 3, 3], strides=[1]), "strides must have 2 entries"),
    ("pads_length", lambda: L(w_of(4, 4), None, (5, 5), off_dims=[18, 3, 3], pads=[1, 1]), "pads must have 4 entries"),
    ("kernel_shape", lambda: L(w_of(4, 4), None, (5, 5), kernel_shape=[3, 3, 3]), "kernel_shape differs"),
    ("stride_0", lambda: L(w_of(4, 4), None, (5, 5), off_dims=[18, 3, 3], strides=[0, 1]), "strides must be >= 1"),
    ("negative_pads", lambda: L(w_of(4, 4), None, (5, 5), off_dims=[18, 3, 3], pads=[-1, 0, 0, 0]), "negative pads"),
    ("dilation_2_21", lambda: L(w_of(4, 4), None, (5, 5), off_dims=[18, 3, 3], dilations=[1 << 21, 1]), "spatial attribute out of range"),
]


@pytest.mark.parametrize("make,why", [r[1:] for r in REFUSALS], ids=[r[0] for r in REFUSALS])
def test_refused_by_node_name(api, tmp_path, make, why):
    with pytest.raises(Exception) as e:
        load_plan(api, tmp_path, make())
    assert "node 'dcn' (DeformConv): unsupported operator form: " in str(e.value) and why in str(e.value), str(e.value)
