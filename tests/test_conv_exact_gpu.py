"""The channel-quad convolution kernels (hip/conv.hip, conv_split.hip) read element by element through the two probes of tests/conv_ref.py, against
its float64 restatement -- not through a GlobalAveragePool, which divides a wrong border pixel by H W before the 1e-4 parity bar sees it.

Exact cases (grid / select / onehot, conv_ref.exact_case) compare bit for bit over the whole map; a failure names the first wrong (row, channel, y, x)
and counts the wrong elements by border / interior and by last 128-pixel block / the others.  Every case asserts from the plan what served it; the
instantiation behind the exec kind follows from conv_ref's restated rules (tests/test_conv_ref.py proves without a GPU that the tables reach them all).

Generic data: every element within conv_ref.error_bound, and the RMS error at most 2 x that of the project's fp32 oracle on the same case (the
margin of the dense tests).  Measured (MI355X; profiles/conv_exact_rms_ratios.txt): 0.87 .. 1.13 over the 24 runs -- the exact-fp32 tiled, weight-stationary,
stem and depthwise kernels 0.89 .. 1.02, the bf16x6 kernels 1.07 .. 1.13 (the stem split6 0.87 .. 0.92), a saturated Tanh 0.36; the worst element
at 0.15 of the bound (depthwise, K = 9) and below 0.005 of it on the deep layers."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

from infera_amd import onnx_writer as W
from tests import conv_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def serve(api, tmp_path, case, weights, xs, probe="A", env=None):
    """the case's graph loaded under its knobs; {rows: served [rows, ...]} and the plan"""
    path = W.write(str(tmp_path / f"{case['id']}-{probe}.onnx"), R.graph(case, weights, probe))
    old = R.set_env(case["env"] if env is None else env)
    try:
        api.load_model("conv_exact", path)
        try:
            plan = api.get_plan("conv_exact")
            out = {r: api.predict_from_blob("conv_exact", np.ascontiguousarray(x, np.float32).tobytes()) for r, x in xs.items()}
        finally:
            api.unload_model("conv_exact")
    finally:
        R.restore_env(old)
    return out, plan, path


def where_wrong(got, want):
    """the first wrong element and the counts by border / interior and by last 128-pixel block / the others"""
    bad = got.view(np.uint32) != want.view(np.uint32)
    if not bad.any():
        return ""
    n, c, y, x = (int(v[0]) for v in np.nonzero(bad))
    N, C, H, Wd = want.shape
    yy, xx = np.meshgrid(np.arange(H), np.arange(Wd), indexing="ij")
    border = ((yy == 0) | (yy == H - 1) | (xx == 0) | (xx == Wd - 1))[None, None]
    pix = (np.arange(N)[:, None, None] * H + yy[None]) * Wd + xx[None]
    last = (pix // 128 == (N * H * Wd - 1) // 128)[:, None]
    return (f"{int(bad.sum())} of {bad.size} wrong; first at (row {n}, channel {c}, y {y}, x {x}): got {got[n, c, y, x]!r}, want {want[n, c, y, x]!r}; "
            f"border {int((bad & border).sum())} / interior {int((bad & ~border).sum())}; last block {int((bad & last).sum())} / other blocks {int((bad & ~last).sum())}")


def run_exact(api, tmp_path, case, env=None):
    got_all = {}
    for kind in case["kinds"]:
        weights, x = R.exact_case(case, kind, max(case["rows"]))
        want = R.assert_exact(case, weights, x, kind)
        out, plan, _ = serve(api, tmp_path, case, weights, {r: x[:r] for r in case["rows"]}, env=env)
        assert plan["activation_layout"] == "NC/4HW4" and plan["exec"] == case["expect"], plan["exec"]
        for r in case["rows"]:
            got = out[r].reshape(r, *want.shape[1:])
            assert not where_wrong(got, want[:r]), (case["id"], kind, r, where_wrong(got, want[:r]))
            got_all[kind, r] = got
    return got_all


@pytest.mark.parametrize("case", R.TILED, ids=lambda c: c["id"])
def test_tiled_fp32_kernel(gpu_api, tmp_path, case):
    run_exact(gpu_api, tmp_path, case)
    print(case["id"], sorted({R.tiled_kernel(*R.conv_under_test(case), R.total_pix(case, r)) for r in case["rows"]}))


@pytest.mark.parametrize("case", R.WS + [R.ws_wrap_case()[0]], ids=lambda c: c["id"])
def test_weight_stationary_kernel_equals_the_reference_and_the_tiled_kernel(gpu_api, tmp_path, case):
    assert R.ws_kernel(*R.conv_under_test(case)[:3]) in R.WS_INSTANCES
    ws = run_exact(gpu_api, tmp_path, case)
    tiled = run_exact(gpu_api, tmp_path, case, env=R.FP32)
    assert all(np.array_equal(ws[k].view(np.uint32), tiled[k].view(np.uint32)) for k in ws)


@pytest.mark.parametrize("case", R.SPLIT, ids=lambda c: c["id"])
def test_bf16x6_split_kernels(gpu_api, tmp_path, case):
    run_exact(gpu_api, tmp_path, case)


@pytest.mark.parametrize("case", R.STEM + R.STEM_POOL, ids=lambda c: c["id"])
def test_stem_kernels(gpu_api, tmp_path, case):
    run_exact(gpu_api, tmp_path, case)


@pytest.mark.parametrize("case", R.NEIGHBOURS, ids=lambda c: c["id"])
def test_neighbouring_channel_quad_kernels(gpu_api, tmp_path, case):
    run_exact(gpu_api, tmp_path, case)


@pytest.mark.parametrize("case", R.AVG, ids=lambda c: c["id"])
def test_average_pools_divide_the_exact_sum(gpu_api, tmp_path, case):
    r = max(case["rows"])
    weights, x = R.exact_case(case, "grid", r)
    want = R.avg_exact(case, weights, x)
    out, plan, _ = serve(gpu_api, tmp_path, case, weights, {r: x})
    assert plan["activation_layout"] == "NC/4HW4" and plan["exec"] == case["expect"], plan["exec"]
    got = out[r].reshape(want.shape)
    assert not where_wrong(got, want), where_wrong(got, want)


@pytest.mark.parametrize("case", [c for c in R.TILED + R.STEM if c["id"] in ("m64-3x3", "c3-m64-5x5-k10")], ids=lambda c: c["id"])
def test_the_two_probes_agree(gpu_api, tmp_path, case):
    """probe A's map at probe B's positions is probe B's output, and probe A on the generic transposed convolution (INFERA_CONVT_MFMA=0) the same bits"""
    idx = R.probe_positions(R.shapes(case)[-1])
    for kind in case["kinds"]:
        r = max(case["rows"])
        weights, x = R.exact_case(case, kind, r)
        want = R.assert_exact(case, weights, x, kind).reshape(r, -1)
        a, plan_a, _ = serve(gpu_api, tmp_path, case, weights, {r: x}, "A")
        b, plan_b, _ = serve(gpu_api, tmp_path, case, weights, {r: x}, "B")
        g, plan_g, _ = serve(gpu_api, tmp_path, case, weights, {r: x}, "A", env=dict(case["env"], INFERA_CONVT_MFMA="0"))
        assert plan_a["exec"][-1] == "convt_phase" and plan_g["exec"][-1] == "normal" and plan_b["activation_layout"] == plan_g["activation_layout"] == "NC/4HW4"
        assert "[rows in channel-quad order]" in plan_b["plan"]["steps"][-1]["origin"]
        assert np.array_equal(a[r].reshape(r, -1).view(np.uint32), want.view(np.uint32)), kind
        assert np.array_equal(b[r].view(np.uint32), want[:, idx].view(np.uint32)), kind
        assert np.array_equal(g[r].view(np.uint32), a[r].view(np.uint32)), kind


@pytest.mark.parametrize("case", R.GENERIC, ids=lambda c: c["id"])
def test_generic_data_within_the_float64_bound(gpu_api, built, tmp_path, case):
    from oracle import oracle

    r = max(case["rows"])
    weights = R.generic_weights(case)
    xs = R.generic_inputs(case, r)
    for name, x in xs.items():
        ref, bound = R.error_bound(case, weights, x)
        out, plan, _ = serve(gpu_api, tmp_path, case, weights, {r: x})
        assert plan["activation_layout"] == "NC/4HW4" and plan["exec"] == case["expect"], plan["exec"]
        got = out[r].reshape(ref.shape).astype(np.float64)
        theirs = oracle.Model(W.write(str(tmp_path / "plain.onnx"), R.graph(case, weights, ""))).predict_blob(x.tobytes()).reshape(ref.shape).astype(np.float64)
        err, err_o = np.abs(got - ref), np.abs(theirs - ref)
        ratio = R.rms(err) / R.rms(err_o) if R.rms(err_o) > 0 else (np.inf if R.rms(err) > 0 else 0.0)
        print(f"{case['id']} {name}: exec {plan['exec']}: worst error / bound = {(err / bound).max():.4f}, oracle's worst / bound = {(err_o / bound).max():.4f}, "
              f"RMS error / the oracle's = {ratio:.3f}")
        assert (err <= bound).all(), (name, float((err / bound).max()))
        assert R.rms(err) <= 2 * R.rms(err_o), (name, ratio)


@pytest.mark.parametrize("name,knob", [("max3x3s2", {"INFERA_POOL_FAST": "0"}), ("stem-split6-7x7s2", {"INFERA_STEM_WAVES": "8"})])
def test_knobs_read_once_per_process(gpu_api, tmp_path, name, knob):
    """INFERA_POOL_FAST=0 (pool2d_cq_kernel in place of pool2d_cq_max_kernel<3, 3>) and INFERA_STEM_WAVES=8 (conv2d_stem_split6_kernel<8>) are read once
    per process: a child of their own runs the case, and must serve the reference's bits -- which the in-process run of the same case serves too"""
    case = next(c for c in R.NEIGHBOURS + R.STEM_POOL if c["id"] == name)
    r = max(case["rows"])
    weights, x = R.exact_case(case, "grid", r)
    want = R.assert_exact(case, weights, x, "grid")
    path = W.write(str(tmp_path / "m.onnx"), R.graph(case, weights))
    np.save(tmp_path / "x.npy", x)
    code = ("import sys, json, numpy as np; sys.path.insert(0, %r); from infera_amd import capi; capi.load_model('m', %r); "
            "y = capi.predict_from_blob('m', np.load(%r).astype(np.float32).tobytes()); np.save(%r, y); print(json.dumps({'exec': capi.get_plan('m')['exec']}))") % (
                ROOT, path, str(tmp_path / "x.npy"), str(tmp_path / "y.npy"))
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **case["env"], **knob), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert json.loads(out.stdout.strip().splitlines()[-1])["exec"] == case["expect"]
    got = np.load(tmp_path / "y.npy").reshape(want.shape)
    assert not where_wrong(got, want), where_wrong(got, want)
