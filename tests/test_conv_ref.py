"""tests/conv_ref.py checked without a GPU: the float64 convolution and pools against torch float64, every exact case proven exact, every case's plan
(made at infera_load_model, no device needed) in channel quads with the exec kinds the case names, and the restated kernel-selection rules reaching
every instantiation the GPU tests claim to cover."""
from __future__ import annotations

import numpy as np
import pytest

from infera_amd import onnx_writer as W
from tests import conv_ref as R

CASES = R.TILED + R.WS + R.SPLIT + R.STEM + R.STEM_POOL + R.NEIGHBOURS + R.AVG + R.GENERIC + [R.ws_wrap_case()[0]]


def _close(a, b):
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max()), np.abs(a - b).max()


@pytest.mark.parametrize("geo", [dict(k=(3, 3), s=1, p=1, d=1, g=1), dict(k=(5, 5), s=2, p=(2, 1, 0, 2), d=1, g=1), dict(k=(3, 2), s=(2, 1), p=(0, 1, 2, 0), d=(2, 1), g=2),
                                 dict(k=(1, 3), s=1, p=(0, 2, 0, 0), d=1, g=1), dict(k=(3, 3), s=1, p=1, d=1, g=8), dict(k=(8, 8), s=1, p=(3, 4, 4, 3), d=1, g=1)],
                         ids=lambda g: "k%dx%d-g%d" % (*g["k"], g["g"]))
def test_conv_reference_agrees_with_torch_float64(geo):
    import torch
    import torch.nn.functional as F

    rng = np.random.default_rng(3)
    x, w, b = rng.standard_normal((2, 8, 11, 9)), rng.standard_normal((16, 8 // geo["g"], *geo["k"])), rng.standard_normal(16)
    p = R._pads(geo["p"])
    xt = F.pad(torch.from_numpy(x), (p[1], p[3], p[0], p[2]))
    want = F.conv2d(xt, torch.from_numpy(w), torch.from_numpy(b), stride=R._pair(geo["s"]), dilation=R._pair(geo["d"]), groups=geo["g"]).numpy()
    _close(R.conv2d64(x, w, b, geo["s"], geo["p"], geo["d"], geo["g"]), want)


@pytest.mark.parametrize("kind,k,s,p,d,ceil,cip", [("max", 3, 2, 1, 1, False, False), ("max", 3, 2, 1, 1, True, False), ("max", 2, 2, 0, 1, True, False),
                                                   ("max", 3, 1, 1, 2, False, False), ("avg", 3, 2, 1, 1, False, False), ("avg", 3, 2, 1, 1, False, True),
                                                   ("avg", 3, 2, 1, 1, True, False), ("avg", 2, 1, 1, 1, False, True), ("avg", 3, 2, 1, 1, True, True)])
def test_pool_reference_agrees_with_torch_float64(kind, k, s, p, d, ceil, cip):
    import torch
    import torch.nn.functional as F

    x = np.random.default_rng(5).standard_normal((2, 4, 12, 10))
    xt = torch.from_numpy(x)
    if kind == "max":
        want = F.max_pool2d(xt, k, s, p, d, ceil_mode=ceil).numpy()
    else:
        want = F.avg_pool2d(xt, k, s, p, ceil_mode=ceil, count_include_pad=cip).numpy()
    _close(R.pool64(x, kind, k, s, p, d, ceil, cip), want)
    # asymmetric pads: the same windows as a symmetric pool of an input torch pads itself (max: -inf; average without pads in the count: zeros that
    # the count must leave out -- checked against a count of ones)
    pads = (1, 0, 0, 1)
    if kind == "max":
        want = F.max_pool2d(F.pad(xt, (pads[1], pads[3], pads[0], pads[2]), value=-np.inf), k, s, 0, d).numpy()
        _close(R.pool64(x, "max", k, s, pads, d), want)
    elif not ceil:
        padded = F.pad(xt, (pads[1], pads[3], pads[0], pads[2]))
        sums = F.avg_pool2d(padded, k, s, 0).numpy() * (k * k)
        ones = F.avg_pool2d(F.pad(torch.ones_like(xt), (pads[1], pads[3], pads[0], pads[2])), k, s, 0).numpy() * (k * k)
        _close(R.pool64(x, "avg", k, s, pads, 1, False, cip), sums / (k * k if cip else ones))


def test_global_pools_activations_and_shuffle():
    import torch

    x = np.random.default_rng(7).standard_normal((2, 12, 5, 7))
    case = {"inp": (12, 5, 7), "ops": [{"op": "gap"}]}
    _close(R.forward64(case, {}, x)["out"], x.mean((2, 3), keepdims=True))
    _close(R.forward64(dict(case, ops=[{"op": "gmp"}]), {}, x)["out"], x.max((2, 3), keepdims=True))
    _close(R.shuffle64(x, 3), torch.nn.functional.channel_shuffle(torch.from_numpy(x), 3).numpy())
    xt = torch.from_numpy(x)
    for kind, want in [("Relu", torch.relu(xt)), ("Sigmoid", torch.sigmoid(xt)), ("Tanh", torch.tanh(xt)), ("LeakyRelu", torch.nn.functional.leaky_relu(xt, float(R.LEAKY))),
                       ("Clip", torch.clamp(xt, float(R.CLIP[0]), float(R.CLIP[1])))]:
        _close(R.act64(x, kind), want.numpy())


@pytest.mark.parametrize("case", [c for c in CASES if c not in R.GENERIC and c not in R.AVG], ids=lambda c: c["id"])
def test_every_exact_case_is_exact(case):
    for kind in case["kinds"]:
        w, x = R.exact_case(case, kind, max(case["rows"]))
        ref = R.assert_exact(case, w, x, kind)
        assert ref.shape[1:] == R.shapes(case)[-1] and np.count_nonzero(ref) > ref.size // 64, kind  # (not a map of zeros)
        if kind != "grid":  # the values a dropped low bit would change are there: most nonzero results use all 24 significand bits
            nz = ref[ref != 0].view(np.uint32)
            assert (nz & 1).mean() > 0.9, kind


@pytest.mark.parametrize("case", R.AVG, ids=lambda c: c["id"])
def test_average_pool_cases_have_exact_sums(case):
    w, x = R.exact_case(case, "grid", max(case["rows"]))
    want = R.avg_exact(case, w, x)
    ref, bound = R.error_bound(case, w, x)
    assert (np.abs(want - ref) <= bound).all()


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["id"])
def test_every_case_plans_in_channel_quads_on_the_expected_kernels(built, tmp_path, case):
    from infera_amd import capi

    w, _ = R.exact_case(case, "grid", 1) if case not in R.GENERIC else (R.generic_weights(case), None)
    probes = ("A", "B") if case["id"] in PROBE_B else ("A",)
    for probe in probes:
        path = W.write(str(tmp_path / f"{probe}.onnx"), R.graph(case, w, probe))
        old = R.set_env(case["env"])
        try:
            capi.load_model("conv_ref_plan", path)
        finally:
            R.restore_env(old)
        try:
            plan = capi.get_plan("conv_ref_plan")
        finally:
            capi.unload_model("conv_ref_plan")
        assert plan["activation_layout"] == "NC/4HW4", plan
        if probe == "A":
            assert plan["exec"] == case["expect"], (plan["exec"], case["expect"])
        else:
            assert plan["exec"][:-1] == case["expect"][:-1] and "[rows in channel-quad order]" in plan["plan"]["steps"][-1]["origin"], plan["exec"]


PROBE_B = ("m64-3x3", "c3-m64-5x5-k10")


@pytest.mark.parametrize("table", ["TILED", "WS", "SPLIT", "STEM", "STEM_POOL", "NEIGHBOURS"])
def test_the_oracle_serves_the_bits_of_every_exact_case(built, tmp_path, table):
    """the project's fp32 oracle (sequential sums, NCHW, no probe: the tensor itself) on the same graphs and inputs: one right answer means it has to
    give the reference's bits too -- graph writer, references and case tables checked against an independent implementation"""
    from oracle import oracle

    for case in getattr(R, table):
        for kind in case["kinds"]:
            r = max(case["rows"])
            w, x = R.exact_case(case, kind, r)
            want = R.assert_exact(case, w, x, kind)
            got = oracle.Model(W.write(str(tmp_path / "m.onnx"), R.graph(case, w, ""))).predict_blob(x.tobytes()).reshape(want.shape)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (case["id"], kind)


# ---- conv2d_generic_kernel<MT>, the NCHW plans and the per-channel operators (tests/test_conv_generic_gpu.py) ----------------------------

NEW_EXACT = R.GENERIC_NCHW + R.GENERIC_CQ + R.NEIGHBOURS_NCHW + R.PER_CHANNEL_EXACT
NEW_CASES = NEW_EXACT + R.AVG_NCHW + R.PER_CHANNEL + R.GENERIC_G + [R.OVER_CAP]
NEW_CASES = NEW_CASES + [R.as_nchw(c) for c in R.GENERIC_CQ_GROUPED + R.PER_CHANNEL_EXACT + R.PER_CHANNEL]  # (the layout bit identity's second run)


@pytest.mark.parametrize("size,C", [(3, 8), (5, 8), (5, 4), (4, 8), (1, 5), (9, 6)])
def test_lrn_reference_agrees_with_torch_float64(size, C):
    """torch pads size // 2 channels in front, ONNX (size - 1) // 2: the same window for an odd size, the mirrored one for an even size"""
    import torch

    x = np.random.default_rng(size).standard_normal((2, C, 3, 4))
    flip = (lambda a: a[:, ::-1].copy()) if size % 2 == 0 else (lambda a: a)
    want = flip(torch.nn.functional.local_response_norm(torch.from_numpy(flip(x)), size, alpha=0.7, beta=0.6, k=1.5).numpy())
    _close(R.lrn64(x, size, 0.7, 0.6, 1.5), want)
    y, sq, base = R.lrn64(x, size, 0.7, 0.6, 1.5, parts=True)
    lo = (size - 1) // 2
    assert np.allclose(sq[:, 0], (x[:, :size - lo] ** 2).sum(1)) and np.allclose(base, 1.5 + 0.7 / size * sq)  # (clipped windows still divide by size)


def test_gate_and_bn_references_agree_with_torch_float64():
    import torch
    import torch.nn.functional as F

    rng = np.random.default_rng(11)
    x = rng.standard_normal((2, 8, 11, 13))
    w, b, s, t = rng.standard_normal((8, 8, 1, 1)), rng.standard_normal(8), rng.standard_normal(8).astype(np.float32), rng.standard_normal(8).astype(np.float32)
    case = {"inp": (8, 11, 13), "ops": [{"op": "gap"}, R.conv(8, 1, act="Sigmoid"), R.gate(0, 2), R.pool("max", 3, 2, 1), R.bn()]}
    r = R.forward64(case, {1: (w, b), 4: (s, t)}, x.reshape(2, -1), bound=True)
    xt = torch.from_numpy(x)
    g = torch.sigmoid(F.conv2d(xt.mean((2, 3), keepdim=True), torch.from_numpy(w), torch.from_numpy(b)))
    _close(r["t"][3], (xt * g).numpy())
    want = F.batch_norm(F.max_pool2d(xt * g, 3, 2, 1), torch.zeros(8, dtype=torch.float64), torch.ones(8, dtype=torch.float64) - 2.0 ** -20, torch.from_numpy(s.astype(np.float64)),
                        torch.from_numpy(t.astype(np.float64)), training=False, eps=2.0 ** -20).numpy()  # (torch wants eps > 0: variance + eps == 1 exactly)
    _close(r["out"], want)
    assert R.shapes(case)[-1] == want.shape[1:] and (r["e"] > 0).all()


@pytest.mark.parametrize("case", [c for c in R.GENERIC_NCHW + R.GENERIC_CQ if c["ops"][-1]["op"] == "conv"], ids=lambda c: c["id"])
def test_grouped_conv_reference_agrees_with_torch_float64_on_the_new_geometries(case):
    import torch
    import torch.nn.functional as F

    o, sh = case["ops"][-1], R.shapes(case)
    C, H, Wd = sh[-2]
    rng = np.random.default_rng(13)
    x, w, b = rng.standard_normal((2, C, H, Wd)), rng.standard_normal((o["M"], C // o["g"], *o["k"])), rng.standard_normal(o["M"])
    p = o["p"]
    want = F.conv2d(F.pad(torch.from_numpy(x), (p[1], p[3], p[0], p[2])), torch.from_numpy(w), torch.from_numpy(b), stride=o["s"], dilation=o["d"], groups=o["g"]).numpy()
    _close(R.conv2d64(x, w, b, o["s"], o["p"], o["d"], o["g"]), want)
    assert want.shape[1:] == sh[-1]


@pytest.mark.parametrize("case", NEW_EXACT, ids=lambda c: c["id"])
def test_every_new_exact_case_is_exact(case):
    assert case["kinds"]
    for kind in case["kinds"]:
        w, x = R.exact_case(case, kind, max(case["rows"]))
        ref = R.assert_exact(case, w, x, kind)
        assert ref.shape[1:] == R.shapes(case)[-1] and np.count_nonzero(ref) > ref.size // 64, kind
        if kind != "grid":
            nz = ref[ref != 0].view(np.uint32)
            assert (nz & 1).mean() > 0.9, kind
        if kind == "onehot" and case["ops"][-1]["g"] > 1:  # every group has its lit pixels: no feature's map is all zeros
            assert (np.abs(ref).sum((0, 2, 3)) > 0).all()
    if case in R.PER_CHANNEL_EXACT and case["ops"][-1]["op"] == "lrn":  # y == x: the reference of the identity IS its input tensor
        r = R.forward64(case, w, x)
        assert np.array_equal(r["t"][-1], r["t"][-2])


@pytest.mark.parametrize("case", R.AVG_NCHW, ids=lambda c: c["id"])
def test_new_average_pool_cases_have_exact_sums(case):
    w, x = R.exact_case(case, "grid", max(case["rows"]))
    want = R.avg_exact(case, w, x)
    ref, bound = R.error_bound(case, w, x)
    assert (np.abs(want - ref) <= bound).all()


@pytest.mark.parametrize("case", NEW_CASES, ids=lambda c: c["id"] + "-" + c["layout"][:4])
def test_every_new_case_plans_in_the_asserted_layout_on_the_asserted_kernels(built, tmp_path, case):
    from infera_amd import capi

    w = R.exact_case(case, "grid", 1)[0] if "grid" in case["kinds"] else R.generic_weights(case)
    path = W.write(str(tmp_path / "m.onnx"), R.graph(case, w, case["probe"]))
    old = R.set_env(case["env"])
    try:
        capi.load_model("conv_ref_plan", path)
    finally:
        R.restore_env(old)
    try:
        plan = capi.get_plan("conv_ref_plan")
    finally:
        capi.unload_model("conv_ref_plan")
    assert plan["activation_layout"] == case["layout"], plan
    if case["expect"] is None:
        assert case["layout"] == "NCHW" and plan["exec"] and all(k == "normal" for k in plan["exec"]), plan["exec"]
    else:
        assert plan["exec"] == case["expect"], (plan["exec"], case["expect"])


@pytest.mark.parametrize("table", ["GENERIC_NCHW", "GENERIC_CQ", "NEIGHBOURS_NCHW", "PER_CHANNEL_EXACT"])
def test_the_oracle_serves_the_bits_of_every_new_exact_case(built, tmp_path, table):
    from oracle import oracle

    for case in getattr(R, table):
        for kind in case["kinds"]:
            r = max(case["rows"])
            w, x = R.exact_case(case, kind, r)
            want = R.assert_exact(case, w, x, kind)
            got = oracle.Model(W.write(str(tmp_path / "m.onnx"), R.graph(case, w, ""))).predict_blob(x.tobytes()).reshape(want.shape)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (case["id"], kind)


def _conv_under_test(case):
    """(C, M, k, groups, the convolution reads the caller's NCHW input) of the case's last convolution"""
    i = max(j for j, o in enumerate(case["ops"]) if o["op"] == "conv")
    o = case["ops"][i]
    return R.shapes(case)[o["src"] if o.get("src") is not None else i][0], o["M"], o["k"], o["g"], i == 0


def test_the_new_tables_reach_every_generic_instantiation_and_edge():
    """from the restated rules (conv.hip conv2d(), schedule.cpp assign_conv_kernels): which instantiation serves each case and why it stays generic"""
    by_id = {c["id"]: c for c in R.GENERIC_NCHW + R.GENERIC_CQ}
    kern = {i: R.generic_kernel(*_conv_under_test(c)[:2], _conv_under_test(c)[3]) for i, c in by_id.items()}
    assert {kern[f"nchw-m{M}"] for M in (1, 5, 32)} == {"conv2d_generic_kernel<1>"} and {kern[f"nchw-m{M}"] for M in (33, 64)} == {"conv2d_generic_kernel<2>"}
    assert {kern[f"nchw-m{M}"] for M in (65, 128, 132, 160)} == {"conv2d_generic_kernel<4>"}
    assert kern["cq-g2-c32-m256-mt4"] == kern["cq-g2-c8-m264-two-tiles"] == kern["cq-stem-c3-m160"] == "conv2d_generic_kernel<4>"
    assert {kern[i] for i in by_id if i.startswith("cq-g4") or i.startswith("cq-g8")} == {"conv2d_generic_kernel<1>"}
    for c in R.GENERIC_CQ:  # every channel-quad case stays on the generic kernel by the restated rule
        C, M, k, g, stem = _conv_under_test(c)
        assert R.generic_served(C, M, k, g, stem), c["id"]
    assert not R.generic_served(8, 8, (3, 3)) and not R.generic_served(8, 8, (3, 3), 8) and R.generic_served(8, 16, (3, 3), 8) and not R.generic_served(3, 32, (3, 3), 1, True)
    KK = {i: (lambda C, M, k, g, _: C // g * k[0] * k[1])(*_conv_under_test(c)) for i, c in by_id.items()}
    assert KK["nchw-kk27"] == 27 and KK["nchw-kk1"] == 1 and KK["nchw-kk5"] == 5 and any(v % 2 for v in KK.values())
    # Mg & 3 != 0 in channel quads (scalar stores into shared quads), Mg == 4 (the 16-byte store), groups that straddle input quads
    Mg = {i: c["ops"][-1]["M"] // c["ops"][-1]["g"] for i, c in by_id.items() if i.startswith("cq-g")}
    assert Mg["cq-g4-c8-m8-shared-quads"] == 2 and Mg["cq-g4-c24-m24-straddling"] == 6 and Mg["cq-g4-c16-m16-quad-store"] == 4 and Mg["cq-g2-c8-m264-two-tiles"] == 132
    # both sides of the cap
    assert KK["nchw-kk8192-cap"] == R.GENERIC_CAP and (lambda C, M, k, g, _: C // g * k[0] * k[1])(*_conv_under_test(R.OVER_CAP)) == R.GENERIC_CAP + 64
    # pixel tails: 35, 105 and 175 pixels -- under one 128-pixel block, one ragged block, images astride a block edge
    assert [r * R.MAP[0] * R.MAP[1] for r in R.ROWS] == [35, 105, 175] and all(c["rows"] == R.ROWS for i, c in by_id.items() if i in ("nchw-m33", "cq-g4-c8-m8-shared-quads"))


def test_the_tables_reach_every_instantiation():
    """from the restated rules (conv.hip conv2d_tiled / launch_ws, conv_split.hip conv2d_split6, conv2d_patch): what each table's launches are"""
    tiled = {R.tiled_kernel(*R.conv_under_test(c), R.total_pix(c, r)) for c in R.TILED for r in c["rows"]}
    assert tiled >= R.TILED_INSTANCES, R.TILED_INSTANCES - tiled
    # a small stride-1 3x3 launch of 128 features falls from MT 4 to MT 2; the 1x1 and stride-2 ones keep MT 4
    by_id = {c["id"]: c for c in R.TILED}
    assert R.tiled_kernel(*R.conv_under_test(by_id["m128-3x3-falls-to-mt2"]), 175) == "conv2d_tiled_kernel<2, 1>"
    assert R.tiled_kernel(*R.conv_under_test(by_id["m128-1x1"]), 175) == "conv2d_tiled_kernel<4, 1>"
    assert R.tiled_kernel(*R.conv_under_test(by_id["c64-m128-3x3s2"]), 175) == "conv2d_tiled_kernel<4, 2>"
    ws = {R.ws_kernel(*R.conv_under_test(c)[:3]) for c in R.WS}
    assert ws == R.WS_INSTANCES, ws ^ R.WS_INSTANCES
    wrap, tiles = R.ws_wrap_case()
    C, M, k, _ = R.conv_under_test(wrap)
    assert R.ws_kernel(C, M, k) == "conv2d_ws_kernel<4, 1, 8>"
    gx, ntiles = R.ws_grid(M, 4, R.total_pix(wrap, 1))
    assert ntiles == tiles == gx * 8 + 1 and R.ws_grid(M, 4, R.total_pix(wrap, 1) - 1)[1] == gx * 8  # one pixel fewer: every wave one tile
    split = {R.split6_kernel(*R.conv_under_test(c)[:3]) for c in R.SPLIT if len(c["ops"]) == 2} | {R.split6_kernel(128, 128, (3, 3), second=True)}
    assert {"conv2d_split6_kernel<2, true>", "conv2d_split6_kernel<2, false>", "conv2d_split6p_kernel[1 stages]", "conv2d_split6p_kernel[2 stages]",
            "conv2d_split6p_kernel[3 stages]", "conv2d_split6p_kernel[36 stages + second input]"} <= split, split
    assert all(R.split6_supported(*R.conv_under_test(c)[:3]) for c in R.SPLIT) and R.split6_takes_second_input(128) and not R.split6_takes_second_input(64)
    assert not R.split6_supported(32, 96, (3, 3)) and not R.split6_supported(40, 64, (1, 1))
    patch = {R.patch_kernel(c["inp"][0], c["ops"][0]["M"], c["ops"][0]["k"]) for c in R.STEM}
    assert {f"conv2d_patch_kernel<{mt}, {k8}>" for mt, k8 in [(1, 0), (2, 0), (1, 4), (2, 10), (3, 19), (4, 0)]} <= patch, patch
    pooled = {R.patch_kernel(c["inp"][0], c["ops"][0]["M"], c["ops"][0]["k"], pool=True) for c in R.STEM_POOL if c["env"].get("INFERA_STEM_POOL2") != "2" and c["env"]}
    assert {"conv2d_patch_kernel<1, 4, true>", "conv2d_patch_kernel<2, 4, true>", "conv2d_patch_kernel<1, 10, true>", "conv2d_patch_kernel<2, 0, true>",
            "conv2d_patch_kernel<2, 19, true>"} <= pooled, pooled
    for c in R.STEM_POOL:
        o = c["ops"][0]
        sh = R.shapes(c)
        assert R.patch_pool_supported(c["inp"][0], o["M"], sh[1][1:], sh[2][1:], c["ops"][1]["p"][0]), c["id"]
        assert R.stem_split6_supported(c["inp"][0], o["M"], o["k"], o["s"]) == (c["expect"][0] == "conv_patch_pool_bf16x6" or "POOL2" in "".join(c["env"]) and o["k"] == (7, 7)), c["id"]
