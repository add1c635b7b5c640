"""GridSample and AffineGrid at load time, without a GPU (INTEGRATION.md 2.6 "Grid sampling"): the plan of each coordinate form, the layouts the
scheduler gives the step, and what is refused, by node name."""
from __future__ import annotations

import numpy as np
import pytest

from infera_amd import onnx_writer as W

CQ, NCHW = "NC/4HW4", "NCHW"
THETA = np.array([1, 0, 0, 0, 1, 0], np.float32)


@pytest.fixture(scope="module")
def api(built):
    from infera_amd import capi

    return capi


def load_plan(api, tmp_path, blob, name="gs"):
    api.load_model(name, W.write(str(tmp_path / f"{name}.onnx"), blob))
    try:
        return api.get_plan(name)
    finally:
        api.unload_model(name)


def kinds(plan):
    return [s["kind"] for s in plan["plan"]["steps"]]


def test_the_stn_is_one_step_without_a_grid(api, tmp_path):
    plan = load_plan(api, tmp_path, W.stn_model(c=1, size=12, mode="bilinear", padding="border", align_corners=0)[0])
    assert kinds(plan) == ["Conv2d", "Pool2d", "Dense", "GridSample", "Conv2d", "GlobalAvgPool", "Dense"]  # (no AffineGrid step: no grid buffer)
    s = plan["plan"]["steps"][3]
    assert (s["coords"], s["mode"], s["padding"], s["align_corners"], s["C"], s["in_hw"], s["out_hw"]) == ("affine", "bilinear", "border", 0, 1, [12, 12], [12, 12])
    assert s["in1"] == plan["plan"]["steps"][2]["out"]  # (it reads the six numbers the Gemm wrote)
    # the warped image stays an image: the plan keeps its channel quads and the step reads and writes NCHW
    assert plan["activation_layout"] == CQ and plan["gridsample"] == [dict(step=3, exec="gridsample_bilinear_nchw", coords="affine", in_layout=NCHW, out_layout=NCHW)]


@pytest.mark.parametrize("order", ["add_first", "transpose_first", "conv"])
def test_a_flow_field_is_read_where_it_lies(api, tmp_path, order):
    """(conv: a convolution writes the field -- the plan is NCHW as a whole, a two-channel tensor is no whole quad)"""
    plan = load_plan(api, tmp_path, W.grid_sample_model("planar", mode="nearest", padding="reflection", align_corners=1, flow_order=order))
    assert kinds(plan)[-2:] == ["BinaryConst", "GridSample"] and "ChannelShuffle" not in kinds(plan)  # (the Add is a step, the Transpose none)
    assert ("Conv2d" in kinds(plan)) == (order == "conv") and plan["activation_layout"] == NCHW
    s = plan["plan"]["steps"][-1]
    assert (s["coords"], s["mode"], s["padding"], s["align_corners"]) == ("planar", "nearest", "reflection", 1) and s["in1"] == plan["plan"]["steps"][-2]["out"]


@pytest.mark.parametrize("kw", [dict(affine_readers=2), dict(affine_align=1)], ids=["two_readers", "other_align_corners"])
def test_a_grid_input_and_an_affine_grid_that_writes_its_grid(api, tmp_path, kw):
    plan = load_plan(api, tmp_path, W.grid_sample_model("grid"))
    assert kinds(plan) == ["SliceCols", "SliceCols", "GridSample"] and plan["plan"]["steps"][2]["coords"] == "grid"
    plan = load_plan(api, tmp_path, W.grid_sample_model("affine", **kw))
    assert kinds(plan)[-2:] == ["AffineGrid", "GridSample"] and plan["plan"]["steps"][-1]["coords"] == "grid"  # (the grid is written, then read)
    assert plan["plan"]["steps"][-2]["out_hw"] == [6, 11] and plan["plan"]["steps"][-1]["in1"] == plan["plan"]["steps"][-2]["out"]


@pytest.mark.parametrize("pre,post,want", [(True, True, ("gridsample_bilinear_cq", CQ, CQ)), (True, False, ("gridsample_bilinear_cq_in", CQ, NCHW)),
                                           (False, True, ("gridsample_bilinear_cq_out", NCHW, CQ))])
def test_the_step_takes_the_layouts_of_its_tensors(api, tmp_path, pre, post, want):
    k = load_plan(api, tmp_path, W.grid_sample_model("affine", c=8, values=THETA, pre=pre, post=post))["gridsample"][0]
    assert (k["exec"], k["in_layout"], k["out_layout"]) == want


REFUSALS = [  # (id, the model, the node, a piece of the reason)
    ("cubic", lambda: W.grid_sample_model("grid", mode="cubic"), "warp", "mode cubic"),
    ("bicubic_opset16", lambda: W.grid_sample_model("grid", mode="bicubic", opset=16), "warp", "mode bicubic"),
    ("volumetric", lambda: W.grid_sample_bare([2, 3, 4, 5], [3, 4, 5, 3]), "warp", "volumetric"),
    ("constant_x", lambda: W.grid_sample_bare([2, 3, 4], [3, 4, 2], x_const=True), "warp", "X is a constant"),
    ("grid_n", lambda: W.grid_sample_bare([2, 3, 5, 7], [3, 4, 4, 2], four_d=True), "warp", "grid's N disagrees"),
    ("grid_last_extent", lambda: W.grid_sample_bare([2, 3, 4], [3, 4, 3]), "warp", "last extent is 3"),
    ("symbolic_hw", lambda: W.grid_sample_bare(["N", 3, "H", "W"], ["N", 4, 4, 2], four_d=True), "warp", "symbolic spatial extents"),
    ("symbolic_ho_wo", lambda: W.grid_sample_bare(["N", 3, 5, 7], ["N", "Ho", "Wo", 2], four_d=True), "warp", "symbolic spatial extents"),
    ("plane_2_31", lambda: W.grid_sample_model("affine", 1, (1 << 16, 1 << 15), (2, 2), values=THETA, loc="gap"), "warp", "2^31"),
    ("extent_2_24", lambda: W.grid_sample_model("affine", 1, ((1 << 24) + 1, 8), (2, 2), values=THETA, loc="gap"), "warp", "above 2^24"),
    ("grid_2_31", lambda: W.grid_sample_model("affine", size=[0, 3, 1 << 16, 1 << 15]), "affine", "2^31"),
    ("quantised", lambda: W.grid_sample_bare([2, 3, 4], [3, 4, 2], quantize=True), "warp", "quantised tensor"),
    ("affine_3d_size", lambda: W.grid_sample_model("affine", size=[0, 3, 4, 5, 6]), "affine", "3-D size"),
    ("affine_dynamic_size", lambda: W.grid_sample_model("affine", size="dynamic"), "affine", "size is not a constant"),
]


@pytest.mark.parametrize("make,node,why", [r[1:] for r in REFUSALS], ids=[r[0] for r in REFUSALS])
def test_refused_by_node_name(api, tmp_path, make, node, why):
    with pytest.raises(Exception) as e:
        load_plan(api, tmp_path, make())
    op = "AffineGrid" if node == "affine" else "GridSample"
    assert f"node '{node}' ({op}): unsupported operator form: " in str(e.value) and why in str(e.value), str(e.value)
