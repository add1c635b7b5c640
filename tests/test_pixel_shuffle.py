"""DepthToSpace, SpaceToDepth and their Reshape -> Transpose -> Reshape spellings without a GPU (INTEGRATION.md 2.6 "Sub-pixel layers"): every
operator form and every spelling lowers to exactly one PixelShuffle step with the expected form, block and output shape; the nodes of a
spelling emit nothing; b = 1 emits no step; the layouts and kernel forms the scheduler chooses for the single layer, the ESPCN model and the
stem; what is refused at load, by node name; and the near misses of a spelling, which are refused where they were before the matcher."""
from __future__ import annotations

import numpy as np
import pytest

from infera_amd import onnx_writer as W

import pixel_shuffle_ref as R

FORM_NAMES = {"dcr": "depth_to_space_dcr", "crd": "depth_to_space_crd", "s2d": "space_to_depth", "unshuffle": "pixel_unshuffle"}
CQ, NCHW = "NC/4HW4", "NCHW"
# the message a 6-D Transpose on an activation has always been refused with
TRANSPOSE_REFUSAL = "on activations only the channel shuffle (0,2,1,3,...) keeps rows independent and is supported"


@pytest.fixture(scope="module")
def api(built):
    from infera_amd import capi

    return capi


def load_plan(api, tmp_path, blob, name="ps"):
    p = W.write(str(tmp_path / f"{name}.onnx"), blob)
    api.load_model(name, p)
    try:
        return api.get_plan(name)
    finally:
        api.unload_model(name)


def kinds(plan):
    return [s["kind"] for s in plan["plan"]["steps"]]


def in_dims(form, b, cs=4, hw=(3, 5)):
    """the input (C, (H, W)) whose spatially larger side is [cs, hw * b]"""
    return (cs * b * b, hw) if form in R.TO_SPACE else (cs, (hw[0] * b, hw[1] * b))


# ---- one layer: the step, its form, block and shapes ----------------------------------------------------------------------------------
LAYERS = [(f, False) for f in ("dcr", "crd", "s2d")] + [(f, True) for f in R.FORMS]


@pytest.mark.parametrize("b", [2, 3, 4])
@pytest.mark.parametrize("form,spelling", LAYERS, ids=[f"{f}-{'spelling' if s else 'op'}" for f, s in LAYERS])
def test_one_layer_is_one_step(api, tmp_path, form, spelling, b):
    c, hw = in_dims(form, b)
    blob, spec = W.pixel_shuffle_model(form, b, c, hw, spelling=spelling)
    plan = load_plan(api, tmp_path, blob)
    assert kinds(plan) == ["PixelShuffle"]  # (the Reshape and Transpose nodes of a spelling emit nothing)
    s = plan["plan"]["steps"][0]
    oc, oh, ow = R.out_shape(form, b, c, *hw)
    assert (s["form"], s["block"], s["C"], s["M"], s["in_hw"], s["out_hw"]) == (FORM_NAMES[form], b, c, oc, list(hw), [oh, ow])
    assert s["bytes_per_row"] == 8 * c * hw[0] * hw[1]  # every element is read once and written once
    assert plan["plan"]["output_shape"] == [-1, oc, oh, ow] and plan["plan"]["flops_per_row"] == 0
    want_origin = "Reshape:ps_split+Transpose:ps_perm+Reshape:ps_merge" if spelling else ("DepthToSpace:ps" if form in R.TO_SPACE else "SpaceToDepth:ps")
    assert s["origin"] == want_origin
    k = plan["pixelshuffle"][0]  # no convolution in the plan: everything stays in the caller's NCHW order, on the generic form
    assert (k["step"], k["kernel"], k["form"], k["block"], k["in_layout"], k["out_layout"]) == (0, "pixelshuffle_generic", FORM_NAMES[form], b, NCHW, NCHW)


def test_depth_to_space_without_mode_is_dcr(api, tmp_path):
    blob, _ = W.pixel_shuffle_model("dcr", 2, 16, (3, 5), mode_attr=False, opset=1)
    assert load_plan(api, tmp_path, blob)["plan"]["steps"][0]["form"] == "depth_to_space_dcr"


@pytest.mark.parametrize("form", R.FORMS)
def test_a_spelling_is_its_operator(api, tmp_path, form):
    """the same step whichever way the layer is written; Shape sub-graphs and -1 in the targets resolve like constants"""
    c, hw = in_dims(form, 2)
    steps = []
    for kw in (dict(spelling=True), dict(spelling=True, lead=-1), dict(spelling=True, target="shape")) + (() if form == "unshuffle" else (dict(),)):
        s = load_plan(api, tmp_path, W.pixel_shuffle_model(form, 2, c, hw, **kw)[0])["plan"]["steps"]
        assert len(s) == 1
        steps.append({k: v for k, v in s[0].items() if k != "origin"})
    assert all(s == steps[0] for s in steps), steps


@pytest.mark.parametrize("form,spelling", LAYERS, ids=[f"{f}-{'spelling' if s else 'op'}" for f, s in LAYERS])
def test_block_one_is_an_alias(api, tmp_path, form, spelling):
    blob, _ = W.pixel_shuffle_model(form, 1, 8, (3, 5), spelling=spelling)
    plan = load_plan(api, tmp_path, blob)
    assert kinds(plan) == [] and plan["plan"]["output_shape"] == [-1, 8, 3, 5]
    blob, _ = W.pixel_shuffle_model(form, 1, 8, (3, 5), spelling=spelling, pre=True, post=True)
    assert kinds(load_plan(api, tmp_path, blob)) == ["Conv2d", "ConvTranspose2d"]


# ---- the scheduler: layouts and kernel forms -------------------------------------------------------------------------------------------
def expected_kernel(form, b, cs, pre, post):
    """the kernel form of a layer whose spatially larger side has cs channels (pre / post: identity 1x1 layers around it)"""
    c = cs * b * b if form in R.TO_SPACE else cs
    oc = R.out_shape(form, b, c, b, b)[0]
    quads = pre and c % 4 == 0 and (not post or oc % 4 == 0)  # the plan is in channel quads
    if not quads:
        return "pixelshuffle_generic", NCHW, NCHW
    if not post:
        return "pixelshuffle_cq_to_nchw", CQ, NCHW
    if form in ("dcr", "s2d"):
        return ("pixelshuffle_quad_copy" if cs % 4 == 0 else "pixelshuffle_generic"), CQ, CQ
    return ("pixelshuffle_transpose" if b in (2, 4) else "pixelshuffle_generic"), CQ, CQ


EMBEDDINGS = {"cq_in_cq_out": dict(pre=True, post=True), "cq_in_nchw_out": dict(pre=True, post=False), "nchw_in_nchw_out": dict(pre=False, post=False)}


@pytest.mark.parametrize("layout", list(EMBEDDINGS))
@pytest.mark.parametrize("cs", [1, 3, 4, 5, 8])
@pytest.mark.parametrize("b", [2, 3, 4])
@pytest.mark.parametrize("form", R.FORMS)
def test_layouts_and_kernel_forms(api, tmp_path, monkeypatch, form, b, cs, layout):
    c, hw = in_dims(form, b, cs)
    emb = EMBEDDINGS[layout]
    blob, _ = W.pixel_shuffle_model(form, b, c, hw, spelling=form == "unshuffle", **emb)
    k = next(iter(load_plan(api, tmp_path, blob)["pixelshuffle"]))
    assert (k["kernel"], k["in_layout"], k["out_layout"]) == expected_kernel(form, b, cs, **emb), k
    monkeypatch.setenv("INFERA_PIXELSHUFFLE_FAST", "0")  # (read when a model is loaded)
    k0 = next(iter(load_plan(api, tmp_path, blob)["pixelshuffle"]))
    assert k0["kernel"] == "pixelshuffle_generic" and (k0["in_layout"], k0["out_layout"]) == (k["in_layout"], k["out_layout"])


@pytest.mark.parametrize("spelling", [False, True], ids=["op", "spelling"])
def test_espcn_stays_in_channel_quads(api, tmp_path, spelling):
    blob, spec = W.espcn(spelling=spelling)
    plan = load_plan(api, tmp_path, blob)
    assert kinds(plan) == ["Conv2d", "Conv2d", "Conv2d", "PixelShuffle"] and plan["activation_layout"] == CQ
    assert plan["exec"][0] == "conv_patch" and all(e.startswith("conv_tiled") or e.startswith("conv_split") for e in plan["exec"][1:3]), plan["exec"]
    k = plan["pixelshuffle"][0]
    assert (k["step"], k["form"], k["block"], k["in_layout"], k["out_layout"], k["kernel"]) == (3, "depth_to_space_crd", 2, CQ, NCHW, "pixelshuffle_cq_to_nchw")
    assert plan["plan"]["output_shape"] == [-1, 3, 24, 24]


def test_stem_reads_the_image_and_writes_channel_quads(api, tmp_path):
    blob, spec = W.pixel_unshuffle_stem()
    plan = load_plan(api, tmp_path, blob)
    assert kinds(plan)[:2] == ["PixelShuffle", "Conv2d"] and plan["activation_layout"] == CQ
    k = plan["pixelshuffle"][0]
    assert (k["form"], k["block"], k["in_layout"], k["out_layout"], k["kernel"]) == ("pixel_unshuffle", 2, NCHW, CQ, "pixelshuffle_nchw_to_cq")
    assert plan["plan"]["steps"][0]["M"] == 12 and plan["exec"][1].startswith(("conv_tiled", "conv_split"))


def test_a_result_without_whole_quads_keeps_the_plan_nchw(api, tmp_path):
    """an internal [N, 5, H, W] tensor behind the shuffle: the plan stays NCHW, as for every other step"""
    blob, _ = W.pixel_shuffle_model("dcr", 2, 20, (3, 5), pre=True, post=True)
    plan = load_plan(api, tmp_path, blob)
    assert plan["activation_layout"] == NCHW and plan["pixelshuffle"][0]["kernel"] == "pixelshuffle_generic"


def test_half_graph_adds_no_rounding(api, tmp_path):
    """a float16 DepthToSpace copies values that are halves already: no RoundHalf behind it"""
    nodes = [W.node("Cast", ["X"], ["xh"], [W.attr_i("to", W.FLOAT16)], name="to_half"),
             W.node("DepthToSpace", ["xh"], ["yh"], [W.attr_i("blocksize", 2)], name="ps"),
             W.node("Cast", ["yh"], ["Y"], [W.attr_i("to", W.FLOAT)], name="to_float")]
    blob = W.model("half_shuffle", nodes, [], [W.value_info("X", ["N", 8, 2, 3])], [W.value_info("Y", ["N", 2, 4, 6])])
    k = kinds(load_plan(api, tmp_path, blob))
    assert k.count("PixelShuffle") == 1 and k[-1] == "PixelShuffle" and k.count("RoundHalf") == 1, k  # (the one rounding is the Cast's)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def op_model(op, attrs, in_dims_, out_dims, opset=13):
    return W.model("refused", [W.node(op, ["X"], ["Y"], attrs, name="ps")], [], [W.value_info("X", ["N"] + list(in_dims_))], [W.value_info("Y", ["N"] + list(out_dims))],
                   opset=opset)


def const_input_model():
    nodes = [W.node("DepthToSpace", ["K"], ["k"], [W.attr_i("blocksize", 2)], name="ps"), W.node("Add", ["X", "k"], ["Y"], name="add")]
    return W.model("refused", nodes, [W.tensor("K", np.zeros((1, 16, 1, 1), np.float32))], [W.value_info("X", ["N", 4, 2, 2])], [W.value_info("Y", ["N", 4, 2, 2])])


def quantised_input_model():
    inits = [W.tensor("s", np.asarray(0.5, np.float32)), W.tensor("z", np.asarray(0, np.uint8))]
    nodes = [W.node("QuantizeLinear", ["X", "s", "z"], ["q"], name="quant"), W.node("DepthToSpace", ["q"], ["qs"], [W.attr_i("blocksize", 2)], name="ps"),
             W.node("DequantizeLinear", ["qs", "s", "z"], ["Y"], name="dequant")]
    return W.model("refused", nodes, inits, [W.value_info("X", ["N", 8, 2, 2])], [W.value_info("Y", ["N", 2, 4, 4])])


REFUSALS = {
    "blocksize_0": (lambda: op_model("DepthToSpace", [W.attr_i("blocksize", 0)], (8, 2, 2), (8, 2, 2)), "blocksize = 0"),
    "blocksize_missing": (lambda: op_model("SpaceToDepth", [], (8, 2, 2), (8, 2, 2)), "blocksize = 0"),
    "c_not_divisible": (lambda: op_model("DepthToSpace", [W.attr_i("blocksize", 2)], (6, 2, 2), (1, 4, 4)), "C = 6 is not divisible by blocksize^2"),
    "c_not_divisible_crd": (lambda: op_model("DepthToSpace", [W.attr_i("blocksize", 3), W.attr_s("mode", "CRD")], (12, 2, 2), (1, 6, 6)), "C = 12 is not divisible by blocksize^2"),
    "h_not_divisible": (lambda: op_model("SpaceToDepth", [W.attr_i("blocksize", 2)], (4, 3, 4), (16, 1, 2)), "H x W = 3 x 4 is not divisible by blocksize = 2"),
    "w_not_divisible": (lambda: op_model("SpaceToDepth", [W.attr_i("blocksize", 3)], (4, 3, 4), (36, 1, 1)), "H x W = 3 x 4 is not divisible by blocksize = 3"),
    "unknown_mode": (lambda: op_model("DepthToSpace", [W.attr_i("blocksize", 2), W.attr_s("mode", "RCD")], (8, 2, 2), (2, 4, 4)), "mode RCD"),
    "constant_input": (const_input_model, "its input is a constant"),
    "rank_3": (lambda: op_model("DepthToSpace", [W.attr_i("blocksize", 2)], (8, 6), (2, 12)), "the input must be an [N,C,H,W] activation"),
    "rank_5": (lambda: op_model("SpaceToDepth", [W.attr_i("blocksize", 2)], (2, 2, 4, 4), (8, 2, 2)), "the input must be an [N,C,H,W] activation"),
    "quantised_input": (quantised_input_model, "it reads the quantised tensor 'q'"),
    "too_many_channels": (lambda: op_model("DepthToSpace", [W.attr_i("blocksize", 2)], (65540, 1, 1), (16385, 2, 2)), "beyond the PixelShuffle kernel's cap"),
    "too_many_channels_out": (lambda: op_model("SpaceToDepth", [W.attr_i("blocksize", 4)], (8192, 4, 4), (131072, 1, 1)), "beyond the PixelShuffle kernel's cap"),
    "plane_too_large": (lambda: op_model("DepthToSpace", [W.attr_i("blocksize", 2)], (4, 1024, 1024), (1, 2048, 2048)), "a plane of more than 2^20 pixels"),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_refused_by_node_name(api, tmp_path, case):
    build, why = REFUSALS[case]
    with pytest.raises(Exception) as e:
        load_plan(api, tmp_path, build())
    msg = str(e.value)
    assert "node 'ps' (" in msg and "unsupported operator form: " in msg and why in msg, msg


def test_symbolic_spatial_extents_are_refused_by_node_name(api, tmp_path):
    blob = op_model("DepthToSpace", [W.attr_i("blocksize", 2)], (8, "H", "W"), (2, "OH", "OW"))
    with pytest.raises(Exception) as e:
        load_plan(api, tmp_path, blob)
    msg = str(e.value)
    assert "node 'ps' (DepthToSpace)" in msg and "unsupported operator form: symbolic spatial extents" in msg, msg


# ---- near misses of a spelling: not absorbed, refused at the Transpose as before ---------------------------------------------------------
NEAR_MISSES = {
    "perm_off_by_one_entry": dict(form="crd", b=2, perm=(0, 1, 4, 2, 3, 5)),
    "perm_of_another_form_s_target": dict(form="dcr", b=2, perm=(0, 1, 4, 2, 5, 3)),
    "unequal_block_extents": dict(form="crd", b=(2, 4)),
    "unequal_block_extents_s2d": dict(form="s2d", b=(1, 2), hw=(3, 6), c=4),
    "second_reader_of_the_6d_value": dict(form="crd", b=2, extra_outputs=["ps_6d"]),
    "second_reader_of_the_transposed_value": dict(form="unshuffle", b=2, extra_outputs=["ps_t"], hw=(6, 10), c=4),
}


@pytest.mark.parametrize("case", list(NEAR_MISSES))
def test_a_near_miss_is_refused_as_before(api, tmp_path, case):
    kw = dict(c=16, hw=(3, 5))
    kw.update(NEAR_MISSES[case])
    blob, _ = W.pixel_shuffle_model(spelling=True, **kw)
    with pytest.raises(Exception) as e:
        load_plan(api, tmp_path, blob)
    msg = str(e.value)
    assert "node 'ps_perm' (Transpose): " + TRANSPOSE_REFUSAL in msg and "PixelShuffle" not in msg, msg
