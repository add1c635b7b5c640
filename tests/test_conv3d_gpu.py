"""conv3d_mfma (staged and direct), conv3d_generic and pool3d (hip/conv3d.hip) against the float64 loop of tests/conv3d_ref.py, each case the
smallest shape at which something specific can go wrong.

Exact: inputs, weights and biases are whole numbers in [-4, 4], so every partial sum is a whole number below 2^24 (asserted of the reference's
sum |x| |w| + |b|): every summation order gives the same f32, and the result equals the reference bit for bit.
Generic data: per element |got - ref| <= (K + 3) 2^-24 (sum |x| |w| + |b|): a K-term f32 dot product in any order, the bias add, the
rounding of the result.  The R(2+1)D pair and the block model are held to the parity bar of the 2-D network tests, 1e-4 |ref| + 1e-6.

The LDS budget case: CC = 8 channels per chunk, so the staged window is 32 E bytes, E = nR kd kh Wpad floats per channel, and fits
kConv3dLdsBudget = 65536 while E <= 2048.  With k = 3, pad 1: Wpad = W + 2 and nR = (62 + W) // W + 1 rows, 2 from W = 63 on: E = 18 (W + 2)
first exceeds 2048 at W = 112 (2052); W = 111 (2034) is the widest staged layer."""
from __future__ import annotations

import os

import numpy as np
import pytest

from infera_amd import onnx_writer as W
from tests import conv3d_ref as R

pytestmark = pytest.mark.gpu

P1 = dict(pads=[1] * 6)
CASES = [  # (id, C, M, (D, H, W), kernel, rows, Conv attributes, plan: exec and, under INFERA_CONV3D_STAGE=1, the input window)
    ("degenerate", 1, 1, (1, 1, 1), (1, 1, 1), 1, {}, ("conv3d_mfma", "lds")),
    ("odd-c-straddle", 3, 5, (4, 5, 6), (3, 3, 3), 2, P1, ("conv3d_mfma", "lds")),
    ("second-channel-tile", 8, 33, (3, 7, 7), (3, 3, 3), 3, P1, ("conv3d_mfma", "lds")),
    ("r3d-stem", 3, 16, (4, 16, 16), (3, 7, 7), 2, dict(strides=[1, 2, 2], pads=[1, 3, 3] * 2), ("conv3d_mfma", "lds")),
    ("tail-chunk", 40, 24, (3, 4, 5), (3, 3, 3), 2, P1, ("conv3d_mfma", "lds")),
    ("odd-tail-chunk", 13, 24, (3, 4, 5), (3, 3, 3), 2, P1, ("conv3d_mfma", "lds")),  # (chunks of 8 channels: 40 is five whole ones, 13 leaves 5 with an odd tail)
    ("asymmetric-dilated", 4, 6, (5, 6, 7), (2, 3, 2), 2, dict(strides=[2, 1, 1], pads=[0, 1, 2, 1, 0, 2], dilations=[2, 1, 2]), ("conv3d_mfma", "lds")),
    ("group2", 8, 8, (3, 5, 5), (3, 3, 3), 2, dict(group=2, **P1), ("conv3d_generic", None)),
    ("depthwise", 8, 8, (3, 5, 5), (3, 3, 3), 2, dict(group=8, **P1), ("conv3d_generic", None)),
    ("over-lds-budget", 8, 4, (1, 2, 112), (3, 3, 3), 2, P1, ("conv3d_mfma", "global")),
    ("widest-staged", 8, 4, (1, 2, 111), (3, 3, 3), 2, P1, ("conv3d_mfma", "lds")),
]
IDS = [c[0] for c in CASES]


def serve(api, tmp_path, blob, x, env=None):
    """the model's result on x [rows, ...] and its plan; env: knobs that are read when the model is loaded"""
    old = {k: os.environ.get(k) for k in env or {}}
    os.environ.update(env or {})
    try:
        api.load_model("c3d", W.write(str(tmp_path / "c3d.onnx"), blob))
    finally:
        for k, v in old.items():
            os.environ.pop(k) if v is None else os.environ.__setitem__(k, v)
    try:
        return api.predict_from_blob("c3d", np.ascontiguousarray(x).tobytes()).reshape(len(x), -1), api.get_plan("c3d")
    finally:
        api.unload_model("c3d")


def layer(case, rng, ints):
    _, c, m, dhw, k, rows, attrs, _ = case
    g = attrs.get("group", 1)
    draw = (lambda *s: rng.integers(-4, 5, size=s).astype(np.float32)) if ints else (lambda *s: rng.standard_normal(s).astype(np.float32))
    return draw(rows, c, *dhw), draw(m, c // g, *k), draw(m)


def ref_of(case, x, w, b):
    a = case[6]
    return R.conv3d(x, w, b, a.get("strides", (1, 1, 1)), a.get("pads", (0,) * 6), a.get("dilations", (1, 1, 1)), a.get("group", 1))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_one_layer_exact_and_within_the_f32_bound(gpu_api, tmp_path, case):
    rng = np.random.default_rng(3)
    for ints in (True, False):
        x, w, b = layer(case, rng, ints)
        ref, mag = ref_of(case, x, w, b)
        blob = W.conv3d_layer(w, b, case[3], **case[6])
        got, plan = serve(gpu_api, tmp_path, blob, x, env={"INFERA_CONV3D_STAGE": "1"})
        s = plan["plan"]["steps"][0]
        assert (s["kind"], s["exec"], s.get("input_window")) == ("Conv3d", *case[7])
        if case[7][1] == "lds":  # the default plan reads its taps from global memory: the same bits
            direct, plan_d = serve(gpu_api, tmp_path, blob, x)
            assert plan_d["plan"]["steps"][0]["input_window"] == "global" and np.array_equal(got, direct)
        got = got.reshape(ref.shape)
        if ints:
            assert mag.max() < 2 ** 24
            assert np.array_equal(got, ref.astype(np.float32)), np.argwhere(got != ref.astype(np.float32))[:4]
        else:
            k = w[0].size
            excess = np.abs(got.astype(np.float64) - ref) / ((k + 3) * 2.0 ** -24 * mag)
            print(case[0], "worst error / bound", excess.max())
            assert excess.max() <= 1.0


def test_staged_and_direct_windows_give_the_same_bits(gpu_api, tmp_path):
    case = CASES[IDS.index("widest-staged")]
    x, w, b = layer(case, np.random.default_rng(5), False)
    blob = W.conv3d_layer(w, b, case[3], act="Relu", **case[6])
    staged, plan_s = serve(gpu_api, tmp_path, blob, x, env={"INFERA_CONV3D_STAGE": "1"})
    direct, plan_d = serve(gpu_api, tmp_path, blob, x)
    generic, plan_g = serve(gpu_api, tmp_path, blob, x, env={"INFERA_CONV3D_MFMA": "0"})
    assert [p["plan"]["steps"][0].get("input_window") for p in (plan_s, plan_d, plan_g)] == ["lds", "global", None]
    assert np.array_equal(staged, direct) and np.count_nonzero(staged) > staged.size // 4
    ref = np.maximum(ref_of(case, x, w, b)[0], 0).reshape(generic.shape)  # (the generic kernel sums in another order: the parity bar, not bits)
    assert (np.abs(generic - ref) <= 1e-4 * np.abs(ref) + 1e-6).all()


def test_a_row_alone_has_the_bits_it_has_in_its_batch(gpu_api, tmp_path):
    case = CASES[IDS.index("second-channel-tile")]
    x, w, b = layer(case[:5] + (5,) + case[6:], np.random.default_rng(7), False)
    blob = W.conv3d_layer(w, b, case[3], **case[6])
    batch, _ = serve(gpu_api, tmp_path, blob, x)
    for r in (0, 4):
        assert np.array_equal(serve(gpu_api, tmp_path, blob, x[r:r + 1])[0], batch[r:r + 1]), r


@pytest.mark.parametrize("ints", [True, False], ids=["exact", "generic"])
def test_r2plus1d_pair(gpu_api, tmp_path, ints):
    blob, w = W.r2plus1d_pair(ints=ints)
    rng = np.random.default_rng(9)
    x = (rng.integers(-4, 5, size=(3, 4, 4, 6, 6)) if ints else rng.standard_normal((3, 4, 4, 6, 6))).astype(np.float32)
    mid, mag1 = R.conv3d(x, w["w1"], w["b1"], pads=(0, 1, 1, 0, 1, 1))
    ref, mag2 = R.conv3d(np.maximum(mid, 0), w["w2"], w["b2"], pads=(1, 0, 0, 1, 0, 0))
    got, plan = serve(gpu_api, tmp_path, blob, x)
    assert [(s["kind"], s.get("act", "")) for s in plan["plan"]["steps"]] == [("Conv3d", "Relu"), ("Conv3d", "")]
    got = got.reshape(ref.shape)
    if ints:
        assert max(mag1.max(), mag2.max()) < 2 ** 24 and np.array_equal(got, ref.astype(np.float32))
    else:
        assert (np.abs(got - ref) <= 1e-4 * np.abs(ref) + 1e-6).all()


POOLS = [("MaxPool", {}), ("MaxPool", dict(ceil_mode=1)), ("AveragePool", {}), ("AveragePool", dict(ceil_mode=1)), ("AveragePool", dict(count_include_pad=1))]


@pytest.mark.parametrize("op,extra", POOLS, ids=[f"{o}-{'-'.join(e) or 'plain'}" for o, e in POOLS])
def test_pool3d(gpu_api, tmp_path, op, extra):
    """k 3, stride 2, pad 1 on 5 x 6 x 7: whole numbers in, so a maximum is exact and an average is one correctly rounded division of an exact sum"""
    x = np.random.default_rng(11).integers(-4, 5, size=(2, 3, 5, 6, 7)).astype(np.float32)
    attrs = dict(kernel_shape=[3, 3, 3], strides=[2, 2, 2], pads=[1] * 6, **extra)
    ref = R.pool3d(x, op, (3, 3, 3), (2, 2, 2), (1,) * 6, extra.get("ceil_mode", 0), extra.get("count_include_pad", 0))
    got, plan = serve(gpu_api, tmp_path, W.pool3d_layer(op, 3, (5, 6, 7), **attrs), x)
    assert plan["plan"]["steps"][0]["kind"] == "Pool3d" and plan["plan"]["output_shape"][1:] == list(ref.shape[1:])
    assert np.array_equal(got.reshape(ref.shape), ref.astype(np.float32))


def test_r3d_block_model_end_to_end(gpu_api, tmp_path):
    blob, ops = W.r3d_net()
    x = np.random.default_rng(13).standard_normal((5, 3, 4, 10, 10)).astype(np.float32)
    ref = R.r3d(ops, x)
    got, plan = serve(gpu_api, tmp_path, blob, x)
    assert plan["activation_layout"] == "NCHW" and got.shape == ref.shape
    assert (np.abs(got - ref) <= 1e-4 * np.abs(ref) + 1e-6).all(), float(np.abs(got - ref).max())
