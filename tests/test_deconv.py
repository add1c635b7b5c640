"""ConvTranspose, Resize and Upsample without a GPU: the float64 references of the writer against torch on the CPU and
against hand-worked tables, the plans of the writer's decoder models (step kinds, fused activations, folded BatchNormalization, layouts,
output shapes, per-phase tap lists, the kernel knob, flops), and what is refused at load."""
from __future__ import annotations

import numpy as np
import pytest

from infera_amd import onnx_writer as W

from deconv_cases import GEOMETRIES, expected_out_hw, geometry


@pytest.fixture(scope="module")
def api(built):
    from infera_amd import capi

    return capi


def load_plan(api, tmp_path, blob, name="dc"):
    p = W.write(str(tmp_path / f"{name}.onnx"), blob)
    api.load_model(name, p)
    try:
        return api.get_plan(name)
    finally:
        api.unload_model(name)


def kinds(plan):
    return [s["kind"] + ("+" + s["act"] if "act" in s else "") for s in plan["plan"]["steps"]]


def rel_err(got, want):
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))


# ---- the references ----------------------------------------------------------------------------------------------------------------
def _torch_conv_transpose(x, w, b, g, one_d):
    """torch in float64; pads that differ between the two ends are cut from the unpadded result (torch pads symmetrically only)"""
    import torch
    import torch.nn.functional as F

    s, d, op = W._pair(g.get("s", 2)), W._pair(g.get("d", 1)), W._pair(g.get("op", 0))
    pt, pl, pb, pr = W._pads4(g.get("p", 0))
    xt, wt, bt = torch.from_numpy(x), torch.from_numpy(w.astype(np.float64)), torch.from_numpy(b.astype(np.float64))
    if one_d:
        y = F.conv_transpose1d(xt, wt, bt, stride=s[1], padding=0, output_padding=op[1], groups=g.get("g", 1), dilation=d[1]).numpy()
        return y[:, :, pl:y.shape[2] - pr]
    y = F.conv_transpose2d(xt, wt, bt, stride=s, padding=0, output_padding=op, groups=g.get("g", 1), dilation=d).numpy()
    return y[:, :, pt:y.shape[2] - pb, pl:y.shape[3] - pr]


@pytest.mark.parametrize("one_d", [False, True], ids=["2d", "1d"])
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_conv_transpose_reference_is_torch(name, one_d):
    g = geometry(name, 8, 12, None if one_d else 5, 7)
    rng = np.random.default_rng(3)
    k = W._pair(g["k"])
    x = rng.normal(size=(2, g["C"], 7) if one_d else (2, g["C"], 5, 7))
    w = rng.normal(size=(g["C"], g["M"] // g.get("g", 1)) + ((k[1],) if one_d else k)).astype(np.float32)
    b = rng.normal(size=g["M"]).astype(np.float32)
    if one_d:
        p4 = W._pads4(g.get("p", 0))
        got = W.conv_transpose_reference(x, w, b, W._pair(g.get("s", 2))[1], (p4[1], p4[3]), W._pair(g.get("d", 1))[1], g.get("g", 1), W._pair(g.get("op", 0))[1])
    else:
        got = W.conv_transpose_reference(x, w, b, g.get("s", 2), g.get("p", 0), g.get("d", 1), g.get("g", 1), g.get("op", 0))
    want = _torch_conv_transpose(x, w, b, g, one_d)
    assert got.shape == want.shape
    assert rel_err(got, want) <= 1e-12


@pytest.mark.parametrize("size", ["x2", "5_to_8"])
@pytest.mark.parametrize("mode,coord,kw", [("nearest", "asymmetric", dict(mode="nearest")), ("linear", "half_pixel", dict(mode="bilinear", align_corners=False)),
                                           ("linear", "align_corners", dict(mode="bilinear", align_corners=True))], ids=["nearest", "half_pixel", "align_corners"])
def test_resize_reference_is_torch_interpolate(mode, coord, kw, size):
    import torch
    import torch.nn.functional as F

    x = np.random.default_rng(5).normal(size=(2, 3, 5, 5))
    out = (10, 10) if size == "x2" else (8, 8)
    want = F.interpolate(torch.from_numpy(x), size=out, **kw).numpy()
    got = W.resize_reference(x, sizes=out, mode=mode, coord=coord, nearest_mode="floor")
    assert rel_err(got, want) <= 1e-12
    if size == "x2":
        assert rel_err(W.resize_reference(x, scales=(2.0, 2.0), mode=mode, coord=coord, nearest_mode="floor"), want) <= 1e-12
    x1 = x[:, :, 0, :]
    want1 = F.interpolate(torch.from_numpy(x1), size=out[1], mode="linear" if mode == "linear" else "nearest", **({} if mode == "nearest" else {"align_corners": kw["align_corners"]})).numpy()
    assert rel_err(W.resize_reference(x1, sizes=(out[1],), mode=mode, coord=coord, nearest_mode="floor"), want1) <= 1e-12


# x_src per output coordinate is worked by hand from the specification's formulas (in the comments), then rounded / split
NEAREST_TABLES = [
    # asymmetric 2 -> 4: x = o / 2 = 0, .5, 1, 1.5
    (2, 4, "asymmetric", "round_prefer_floor", [0, 0, 1, 1]), (2, 4, "asymmetric", "round_prefer_ceil", [0, 1, 1, 1]),
    (2, 4, "asymmetric", "floor", [0, 0, 1, 1]), (2, 4, "asymmetric", "ceil", [0, 1, 1, 1]),
    # half_pixel 3 -> 6: x = (o + .5) / 2 - .5 = -.25, .25, .75, 1.25, 1.75, 2.25
    (3, 6, "half_pixel", "floor", [0, 0, 0, 1, 1, 2]), (3, 6, "half_pixel", "ceil", [0, 1, 1, 2, 2, 2]),
    (3, 6, "half_pixel", "round_prefer_floor", [0, 0, 1, 1, 2, 2]), (3, 6, "pytorch_half_pixel", "round_prefer_ceil", [0, 0, 1, 1, 2, 2]),
    # align_corners 3 -> 5: x = o * 2 / 4 = 0, .5, 1, 1.5, 2
    (3, 5, "align_corners", "round_prefer_floor", [0, 0, 1, 1, 2]), (3, 5, "align_corners", "round_prefer_ceil", [0, 1, 1, 2, 2]),
    # one output coordinate: pytorch_half_pixel reads x = 0, half_pixel x = .5 * 3 - .5 = 1
    (3, 1, "pytorch_half_pixel", "floor", [0]), (3, 1, "half_pixel", "floor", [1]), (3, 1, "align_corners", "floor", [0]),
]


@pytest.mark.parametrize("n_in,n_out,coord,nearest_mode,want", NEAREST_TABLES)
def test_resize_reference_nearest_tables(n_in, n_out, coord, nearest_mode, want):
    assert W.resize_axis_reference(n_in, n_out, n_out / n_in, "nearest", coord, nearest_mode).tolist() == want
    x = np.arange(2 * n_in, dtype=np.float64).reshape(1, 2, n_in)
    assert np.array_equal(W.resize_reference(x, sizes=(n_out,), mode="nearest", coord=coord, nearest_mode=nearest_mode), x[:, :, want])


LINEAR_TABLES = [
    # asymmetric 2 -> 4: x = 0, .5, 1, 1.5 -> clamped to 1
    (2, 4, "asymmetric", [(0, 1, 0.0), (0, 1, 0.5), (1, 1, 0.0), (1, 1, 0.0)]),
    # half_pixel 2 -> 4: x = -.25 -> 0, .25, .75, 1.25 -> 1
    (2, 4, "half_pixel", [(0, 1, 0.0), (0, 1, 0.25), (0, 1, 0.75), (1, 1, 0.0)]),
    (2, 4, "pytorch_half_pixel", [(0, 1, 0.0), (0, 1, 0.25), (0, 1, 0.75), (1, 1, 0.0)]),
    # align_corners 4 -> 7: x = o / 2
    (4, 7, "align_corners", [(0, 1, 0.0), (0, 1, 0.5), (1, 2, 0.0), (1, 2, 0.5), (2, 3, 0.0), (2, 3, 0.5), (3, 3, 0.0)]),
    (3, 1, "pytorch_half_pixel", [(0, 1, 0.0)]), (3, 1, "half_pixel", [(1, 2, 0.0)]),
]


@pytest.mark.parametrize("n_in,n_out,coord,want", LINEAR_TABLES)
def test_resize_reference_linear_tables(n_in, n_out, coord, want):
    i0, i1, w = W.resize_axis_reference(n_in, n_out, n_out / n_in, "linear", coord)
    assert list(zip(i0.tolist(), i1.tolist(), w.tolist())) == want


# ---- plans -------------------------------------------------------------------------------------------------------------------------
def test_autoencoder_plan(api, tmp_path):
    blob, spec = W.conv_autoencoder((3, 16, 32), 16)
    plan = load_plan(api, tmp_path, blob)
    assert kinds(plan) == ["Conv2d+Relu", "Conv2d+Relu", "ConvTranspose2d+Relu", "ConvTranspose2d+Sigmoid"]  # (no BatchNormalization step: folded)
    assert "BatchNormalization" in plan["plan"]["steps"][2]["origin"]
    assert plan["plan"]["output_shape"] == [-1, 3, 16, 16]
    assert plan["activation_layout"] == "NC/4HW4"
    assert [(c["kernel"], c["in_layout"], c["out_layout"]) for c in plan["convt"]] == [("convt2d_phase", "NC/4HW4", "NC/4HW4"), ("convt2d_phase", "NC/4HW4", "NCHW")]
    assert plan["exec"][2:] == ["convt_phase", "convt_phase"]
    # per image: two stride-2 convolutions and two transposed ones, 2 * C * M * kh * kw * H * W each for the latter
    assert plan["plan"]["flops_per_row"] == 2 * (27 * 16 * 64 + 144 * 32 * 16) + 2 * (32 * 16 * 16 * 16 + 16 * 3 * 16 * 64)


def test_unet_stays_in_channel_quads_until_the_last_layer(api, tmp_path):
    blob, _ = W.unet_small(3, 3, 16)
    plan = load_plan(api, tmp_path, blob)
    assert kinds(plan) == ["Conv2d+Relu", "Conv2d+Relu", "Conv2d+Relu", "ConvTranspose2d+Relu", "CopyCols", "CopyCols", "Conv2d+Relu", "ConvTranspose2d"]
    assert plan["activation_layout"] == "NC/4HW4"
    assert [(c["in_layout"], c["out_layout"]) for c in plan["convt"]] == [("NC/4HW4", "NC/4HW4"), ("NC/4HW4", "NCHW")]
    assert plan["plan"]["output_shape"] == [-1, 3, 16, 16]


def test_upsample_decoder_and_conv1d_autoencoder_plans(api, tmp_path):
    plan = load_plan(api, tmp_path, W.upsample_decoder((8, 4, 4), 3)[0])
    assert kinds(plan) == ["Resize2d", "Conv2d+Relu", "Resize2d", "Conv2d"]
    r = plan["plan"]["steps"][0]
    assert (r["mode"], r["coordinate_transformation_mode"], r["nearest_mode"], r["in_hw"], r["out_hw"]) == ("nearest", "asymmetric", "floor", [4, 4], [8, 8])
    assert plan["plan"]["output_shape"] == [-1, 3, 16, 16]
    plan = load_plan(api, tmp_path, W.conv1d_autoencoder(16, 4)[0])
    assert kinds(plan) == ["Conv2d+Relu", "Conv2d+Relu", "ConvTranspose2d+Relu", "ConvTranspose2d", "BinaryAct", "RowReduce"]
    assert plan["plan"]["steps"][3]["in_hw"] == [1, 8] and plan["plan"]["steps"][3]["out_hw"] == [1, 16]
    assert plan["plan"]["output_shape"] == [-1]
    # the reconstruction meets the table's flat columns element by element: the last layer stores NCHW, the plan before it stays in channel quads
    assert plan["activation_layout"] == "NC/4HW4"
    assert [(c["kernel"], c["in_layout"], c["out_layout"]) for c in plan["convt"]] == [("convt2d_phase", "NC/4HW4", "NC/4HW4"), ("convt2d_phase", "NC/4HW4", "NCHW")]


def brute_force_phases(s):
    """Per phase: the output pixels that belong to it and the taps that reach them, by enumeration over (oh, ky) and (ow, kx)."""
    (kh, kw), (sh, sw), (dh, dw), (pt, pl) = s["k"], s["strides"], s["dilations"], s["pads"][:2]
    (H, Wd), (OH, OW) = s["in_hw"], s["out_hw"]

    def axis(n_in, n_out, k, st, d, p):
        out = []
        for ph in range(st):
            os_ = [o for o in range(n_out) if (o + p) % st == ph]
            # a tap reaches the phase when SOME input coordinate (inside the image or not: the kernels mask) maps onto its pixels
            taps = [t for t in range(k) if (ph - t * d) % st == 0]
            for o in os_:
                assert {t for t in range(k) if (o + p - t * d) % st == 0} == set(taps)
                for t in range(k):
                    if (o + p - t * d) % st == 0 and 0 <= (o + p - t * d) // st < n_in:
                        assert t in taps
            # the input coordinate of the phase's j-th pixel through tap t is j + q, by the definition ih = (o + p - t d) / s of every pixel
            qs = [(ph - t * d) // st + ((os_[0] + p - ph) // st if os_ else 0) for t in taps]
            for j, o in enumerate(os_):
                for t, q in zip(taps, qs):
                    assert (o + p - t * d) // st == j + q
            out.append((os_[0] if os_ else None, len(os_), taps, qs))
        return out

    want = []
    for a, (h0, hn, ht, hq) in enumerate(axis(H, OH, kh, sh, dh, pt)):
        for b, (w0, wn, wt, wq) in enumerate(axis(Wd, OW, kw, sw, dw, pl)):
            want.append({"phase": [a, b], "pixels": [hn, wn], "taps": [[y, x] for y in ht for x in wt], "first": [h0, w0],
                         "source_offsets": [[y, x] for y in hq for x in wq]})
    return want


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_output_shapes_and_phase_tap_lists(api, tmp_path, name):
    g = geometry(name, 8, 12, 5, 7)
    blob, spec = W.conv_transpose_model(g)
    plan = load_plan(api, tmp_path, blob)
    (s,) = plan["plan"]["steps"]
    assert s["kind"] == "ConvTranspose2d" and s["out_hw"] == list(expected_out_hw(g)) == list(spec["out_shape"][1:])
    assert plan["plan"]["output_shape"] == [-1, g["M"]] + s["out_hw"]
    assert (s["C"], s["M"], s["group"], s["in_hw"]) == (8, g["M"], g.get("g", 1), [5, 7])
    got = s["phases"]
    want = brute_force_phases(s)
    assert len(got) == len(want) == s["strides"][0] * s["strides"][1]
    for gp, wp in zip(got, want):
        assert gp["phase"] == wp["phase"] and gp["pixels"] == wp["pixels"] and gp["taps"] == wp["taps"]
        if wp["pixels"][0] and wp["pixels"][1]:
            assert gp["first"] == wp["first"] and gp["source_offsets"] == wp["source_offsets"]
    assert sum(len(p["taps"]) for p in got) == s["k"][0] * s["k"][1]  # every tap belongs to exactly one phase
    assert plan["plan"]["flops_per_row"] == 2 * (8 // g.get("g", 1)) * g["M"] * s["k"][0] * s["k"][1] * 5 * 7
    # the 1-D form runs as [N, C, 1, L]
    g1 = geometry(name, 8, 12, None, 7)
    (s1,) = load_plan(api, tmp_path, W.conv_transpose_model(g1)[0])["plan"]["steps"]
    assert s1["in_hw"] == [1, 7] and s1["out_hw"] == list(expected_out_hw(g1)) and s1["k"][0] == 1


@pytest.mark.parametrize("auto_pad,output_shape,pads,out_hw", [
    # total = s (H - 1) + op + (k - 1) d + 1 - output_shape = 2 * 4 + 0 + 2 + 1 - 10 = 1 on both axes: the larger half first unless SAME_UPPER
    ("NOTSET", (10, 10), [1, 1, 0, 0], [10, 10]),
    ("SAME_UPPER", None, [0, 0, 1, 1], [10, 10]),
    ("SAME_LOWER", None, [1, 1, 0, 0], [10, 10]),
    ("SAME_UPPER", (9, 10), [1, 0, 1, 1], [9, 10]),
    ("VALID", None, [0, 0, 0, 0], [11, 11]),
])
def test_output_shape_and_auto_pad(api, tmp_path, auto_pad, output_shape, pads, out_hw):
    g = dict(C=4, M=4, H=5, W=5, k=3, s=2, auto_pad=auto_pad, output_shape=output_shape)
    blob, spec = W.conv_transpose_model(g)
    (s,) = load_plan(api, tmp_path, blob)["plan"]["steps"]
    assert s["pads"] == pads and s["out_hw"] == out_hw == list(spec["out_shape"][1:])


def test_knob_changes_the_kernel_and_nothing_else(api, tmp_path, monkeypatch):
    blob, _ = W.conv_transpose_model(geometry("k4_s2_p1", 32, 32, 5, 5), pre=True, post=True, act="Relu")
    on = load_plan(api, tmp_path, blob)
    monkeypatch.setenv("INFERA_CONVT_MFMA", "0")
    off = load_plan(api, tmp_path, blob)
    assert [c["kernel"] for c in on["convt"]] == ["convt2d_phase", "convt2d_phase"]
    assert [c["kernel"] for c in off["convt"]] == ["convt2d_generic", "convt2d_generic"]
    assert on["exec"] == ["normal", "convt_phase", "convt_phase"] and off["exec"] == ["normal", "normal", "normal"]
    for c in on["convt"] + off["convt"]:
        del c["kernel"]
    del on["exec"], off["exec"]
    assert on == off
    # grouped layers and channel counts that are not whole quads run on the generic kernel either way
    monkeypatch.delenv("INFERA_CONVT_MFMA")
    for g in (geometry("groups4", 32, 32, 5, 5), geometry("k2_s2", 3, 8, 5, 5)):
        plan = load_plan(api, tmp_path, W.conv_transpose_model(g, pre=True, post=True)[0])
        assert plan["convt"][0]["kernel"] == "convt2d_generic"


def test_batchnorm_and_affine_fold_and_activation_fuse(api, tmp_path):
    plan = load_plan(api, tmp_path, W.conv_transpose_model(geometry("k2_s2", 8, 8, 4, 4), bn=True, act="Tanh")[0])
    assert kinds(plan) == ["ConvTranspose2d+Tanh"]
    # kinds beyond 1..5 stay an elementwise step
    plan = load_plan(api, tmp_path, W.conv_transpose_model(geometry("k2_s2", 8, 8, 4, 4), act="Softplus")[0])
    assert kinds(plan) == ["ConvTranspose2d", "Unary+Softplus"]


# ---- rejections --------------------------------------------------------------------------------------------------------------------
def _raw_convt(attrs=(), w_shape=(4, 4, 3, 3), x_dims=("N", 4, 5, 5), inputs=("X", "W", "B"), b_len=4, op="ConvTranspose"):
    inits = [W.tensor("W", np.ones(w_shape, np.float32)), W.tensor("B", np.ones(b_len, np.float32))]
    return W.model("bad", [W.node(op, list(inputs), ["Y"], list(attrs), name="up")], inits, [W.value_info("X", list(x_dims))], [W.value_info("Y", ["N", 4, "h", "w"])])


CONVT_REJECTIONS = {
    "non_constant_W": (dict(inputs=("X", "X")), "W must be a constant"),
    "non_constant_B": (dict(inputs=("X", "W", "X")), "B must be a constant"),
    "output_padding_stride": (dict(attrs=[W.attr_ints("strides", [2, 2]), W.attr_ints("output_padding", [2, 0])]), "output_padding must be smaller than max(stride, dilation)"),
    "output_padding_no_stride": (dict(attrs=[W.attr_ints("output_padding", [0, 1])]), "output_padding must be smaller than max(stride, dilation)"),
    "negative_pads_attr": (dict(attrs=[W.attr_ints("pads", [0, -1, 0, 0])]), "negative pads"),
    "negative_pads_output_shape": (dict(attrs=[W.attr_ints("output_shape", [9, 9])]), "negative pads"),
    "negative_extent": (dict(attrs=[W.attr_ints("pads", [4, 4, 4, 4])]), "negative extents"),
    "rank_5": (dict(x_dims=("N", 4, 5, 5, 5), w_shape=(4, 4, 3, 3, 3)), "rank 3 or 4"),
    "rank_2": (dict(x_dims=("N", 4), w_shape=(4, 4)), "rank 3 or 4"),
    "C_mod_group": (dict(attrs=[W.attr_i("group", 3)]), "not a multiple of group"),
    "weight_shape": (dict(w_shape=(8, 4, 3, 3)), "disagrees with C = 4"),
    "bias_size": (dict(b_len=5), "B has 5 entries"),
    "kernel_cap": (dict(w_shape=(4, 4, 65, 1)), "kernel extents must be 1..64"),
}


@pytest.mark.parametrize("case", list(CONVT_REJECTIONS))
def test_conv_transpose_rejections(api, tmp_path, case):
    kw, why = CONVT_REJECTIONS[case]
    with pytest.raises(api.InferaError) as e:
        load_plan(api, tmp_path, _raw_convt(**kw))
    assert "node 'up' (ConvTranspose): unsupported operator form: " in str(e.value) and why in str(e.value), str(e.value)


RESIZE_REJECTIONS = {
    "cubic": (dict(mode="cubic"), "cubic"),
    "tf_crop_and_resize": (dict(coord="tf_crop_and_resize"), "tf_crop_and_resize"),
    "antialias": (dict(attrs_extra=[W.attr_i("antialias", 1)], opset=18), "antialias = 1"),
    "exclude_outside": (dict(attrs_extra=[W.attr_i("exclude_outside", 1)]), "exclude_outside = 1"),
    "keep_aspect_ratio_policy": (dict(attrs_extra=[W.attr_s("keep_aspect_ratio_policy", "not_larger")], opset=18), "keep_aspect_ratio_policy not_larger"),
    "scale_N": (dict(lead=(2.0, 1.0)), "scaling of the N or C axis"),
    "scale_C": (dict(lead=(1.0, 2.0)), "scaling of the N or C axis"),
}


@pytest.mark.parametrize("case", list(RESIZE_REJECTIONS))
def test_resize_rejections(api, tmp_path, case):
    kw, why = RESIZE_REJECTIONS[case]
    net = W._DecoderNet(0)
    args = dict(scales=(2.0, 2.0), mode="nearest", coord="half_pixel")
    args.update(kw)
    opset = args.pop("opset", 13)
    out = net.resize("X", 4, **args, opset=opset)
    blob = W.model("bad", net.nodes, net.inits, [W.value_info("X", ["N", 4, 5, 5])], [W.value_info(out, ["N", 4, "h", "w"])], opset=opset)
    with pytest.raises(api.InferaError) as e:
        load_plan(api, tmp_path, blob)
    assert "node 'resize1' (Resize): unsupported operator form: " in str(e.value) and why in str(e.value), str(e.value)


def test_sizes_that_scale_channels_are_refused(api, tmp_path):
    with pytest.raises(api.InferaError, match="scaling of the N or C axis"):
        load_plan(api, tmp_path, W.resize_model(4, (5, 5), sizes=(8, 8), lead=(0, 8))[0])


# ---- Upsample ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["nearest", "linear"])
@pytest.mark.parametrize("opset", [7, 9])
def test_upsample_gives_the_plan_of_its_resize_twin(api, tmp_path, mode, opset):
    up = load_plan(api, tmp_path, W.resize_model(4, (5, 6), scales=(2.0, 3.0), mode=mode, op="Upsample", opset=opset)[0])
    twin = load_plan(api, tmp_path, W.resize_model(4, (5, 6), scales=(2.0, 3.0), mode=mode, coord="asymmetric", nearest_mode="floor", opset=13)[0])
    old = load_plan(api, tmp_path, W.resize_model(4, (5, 6), scales=(2.0, 3.0), mode=mode, opset=10)[0])
    for p in (up, twin, old):
        for s in p["plan"]["steps"]:
            s["origin"] = s["origin"].replace("Upsample", "Resize")
    assert up == twin == old
    assert up["plan"]["steps"][0]["out_hw"] == [10, 18]


def test_resize_1d_and_sizes(api, tmp_path):
    (s,) = load_plan(api, tmp_path, W.resize_model(3, (5,), sizes=(8,), mode="linear", coord="align_corners")[0])["plan"]["steps"]
    assert (s["kind"], s["mode"], s["coordinate_transformation_mode"], s["in_hw"], s["out_hw"]) == ("Resize2d", "linear", "align_corners", [1, 5], [1, 8])
    (s,) = load_plan(api, tmp_path, W.resize_model(8, (7,), scales=(2.0,), mode="linear", coord="half_pixel")[0])["plan"]["steps"]
    assert (s["mode"], s["in_hw"], s["out_hw"]) == ("linear", [1, 7], [1, 14])
