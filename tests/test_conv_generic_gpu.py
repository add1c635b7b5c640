"""conv2d_generic_kernel<MT> (hip/conv.hip) and the NCHW forms of its neighbours (pool2d_kernel, the NCHW branches of global_avgpool_kernel,
channel_shuffle_planes_kernel<false>, copy_cols, lrn_kernel, gate_planes_kernel, affine_planes_kernel) element by element against the float64
restatement of tests/conv_ref.py -- the layers tests/test_conv_exact_gpu.py does not reach: every convolution of a plan that stays NCHW, and inside
channel-quad plans every convolution the fast kernels refuse.  Every case asserts the layout of its plan and the exec kind of every step, so a change
to conv2d()'s choice of MT (restated as conv_ref.generic_kernel, checked without a GPU in tests/test_conv_ref.py) or to decide_layout shows as a
failed assertion about what served the case, not as lost coverage.

GENERIC_NCHW -- one convolution of the caller's input served as the tensor itself (probe ""): plan "NCHW", every step "normal".
  nchw-m1 .. m160      feature tiles by Mg = M / groups: <1> to 32, <2> to 64, <4> beyond; 33, 65 and 132 leave a tile almost empty, 132 and 160 take
                       two workgroups of features.  Rows 1 / 3 / 5 of a 5 x 7 map are 35 / 105 / 175 pixels: under one 128-pixel block, a ragged
                       block, images astride a block edge
  nchw-kk27, kk1, kk5  the k loop takes two taps per step, one per lane half: an odd KK = Cg kh kw (and KK = 1) leaves the upper half on `k < KK`
  nchw-3x3d2 .. 2x2    the corner pointer xc before the image under dilation, stride, asymmetric pads, a 9x9 window larger than the 5 x 7 map
  nchw-g3 .. g6        the input channel grp * Cg + c: Cg = Mg = 2; Cg = 4, Mg = 6; a depth multiplier; depthwise where the plan is NCHW
  nchw-relu .. nobias  the epilogues that are exact on a grid (Sigmoid and Tanh: GENERIC_G)
  nchw-kk8192-cap      the k table fills the 64 KiB of LDS exactly; OVER_CAP (KK = 8256) is refused when the model is loaded, naming 8192.  (A
                       [4, 1, 1] result has no layout: this plan is in channel quads, its one step the generic kernel -- asserted as such.)
GENERIC_CQ -- probe A, plan "NC/4HW4", the convolution under test "normal" behind the 8 -> C 1x1 stem (conv_patch).
  cq-g4-c8-m8          Cg = Mg = 2: two groups in one input quad, `Mg & 3 != 0` sends every store down the scalar path into quads two groups share
  cq-g4-c24-m24        Cg = Mg = 6: groups straddle quads on both sides
  cq-g4-c16-m16        Mg = 4: the 16-byte store at grp * Mg + ml
  cq-g2-c32-m256       Mg = 128: <4>;  cq-g2-c8-m264: Mg = 132, two feature workgroups per group;  cq-g8-c8-m16: a depth multiplier of 2
  cq-9x9-81-taps       more taps than the tiled kernel's 64-bit mask
  cq-stem-*            stems the patch kernel refuses (C > 8, M > 128, groups > 1): NCHW in, channel quads out
  cq-head-m10          a 1x1 convolution on the [C, 1, 1] of a global pool, 10 features stored in plain order
NEIGHBOURS_NCHW, AVG_NCHW -- the geometries of NEIGHBOURS and AVG behind a 6-channel stem (not whole quads) or a slice off a quad boundary.
PER_CHANNEL_EXACT, PER_CHANNEL -- LRN (sizes 3, 5, 4; 5 on 4 channels: the window clipped at both ends), the squeeze-and-excitation gate and a
BatchNormalization behind a max pool, each in channel quads (probe A) and in NCHW (probe "").

Exact kinds bit for bit.  The two layouts give the same bits on generic data too: the generic kernel's k order and the operation order of lrn / gate
/ bn do not depend on the layout (the layers in front of them, served by different kernels in the two plans, get selection weights there: one term
per sum).  Generic data (GENERIC_G): every element within conv_ref.error_bound, the RMS error at most 2 x the fp32 oracle's, a row alone the bits it
has inside its batch.  LRN's generic data is held to the parity bar |got - ref| <= 1e-4 |ref| + 1e-6 against float64: neither device_common.hpp nor
the ROCm documents give a figure for the device's powf; gate and bn to their derived terms.

Probe A hands a -0.0 on as +0.0 (the other channels' 0 * x added to 1 * x; conv_ref.through_probe): the gate of a negative value by zero is -0.0, and
the NCHW run of the same case, served as it is, holds the sign too.

Measured (MI355X; profiles/conv_generic_rms_ratios.txt), 42 runs.  The generic kernel on generic data: RMS error 0.89 .. 1.05 of the fp32 oracle's
(1.000 where the plan is NCHW and K is small: the same sums), the worst element at 0.079 of the bound (Sigmoid, K = 54) and 0.002 on the 9x9 filter.
LRN: the worst element at 0.0008 .. 0.0018 of the parity bar, RMS 0.97 .. 1.17 of the oracle's, the same figures in both layouts.  Gate: 0.11 of its
bound; the unfolded BatchNormalization: 0.27 (a two-rounding bound on a multiply and an add); RMS 0.87 .. 1.00 of the oracle's."""
from __future__ import annotations

import numpy as np
import pytest

from infera_amd import onnx_writer as W
from tests import conv_ref as R
from tests.test_conv_exact_gpu import serve, where_wrong

pytestmark = pytest.mark.gpu


def check_plan(case, plan):
    assert plan["activation_layout"] == case["layout"], (case["id"], plan["activation_layout"])
    if case["expect"] is None:
        assert plan["exec"] and all(k == "normal" for k in plan["exec"]), (case["id"], plan["exec"])
    else:
        assert plan["exec"] == case["expect"], (case["id"], plan["exec"])


def run_exact(api, tmp_path, case, want_of=R.assert_exact):
    for kind in case["kinds"]:
        weights, x = R.exact_case(case, kind, max(case["rows"]))
        want = R.through_probe(want_of(case, weights, x, kind), case["probe"])
        out, plan, _ = serve(api, tmp_path, case, weights, {r: x[:r] for r in case["rows"]}, probe=case["probe"])
        check_plan(case, plan)
        for r in case["rows"]:
            got = out[r].reshape(r, *want.shape[1:])
            assert not where_wrong(got, want[:r]), (case["id"], kind, r, where_wrong(got, want[:r]))


def last_conv(case):
    i = max(j for j, o in enumerate(case["ops"]) if o["op"] == "conv")
    o = case["ops"][i]
    return R.shapes(case)[o["src"] if o.get("src") is not None else i][0], o["M"], o["g"]


@pytest.mark.parametrize("case", R.GENERIC_NCHW, ids=lambda c: c["id"])
def test_generic_kernel_in_an_nchw_plan(gpu_api, tmp_path, case):
    run_exact(gpu_api, tmp_path, case)
    print(case["id"], R.generic_kernel(*last_conv(case)))


@pytest.mark.parametrize("case", R.GENERIC_CQ, ids=lambda c: c["id"])
def test_generic_kernel_in_a_channel_quad_plan(gpu_api, tmp_path, case):
    run_exact(gpu_api, tmp_path, case)
    print(case["id"], R.generic_kernel(*last_conv(case)))


def test_a_convolution_over_the_lds_cap_is_refused_at_load(gpu_api, tmp_path):
    """KK = 516 x 4 x 4 = 8256 > 8192 (its neighbour with 8192 is served: nchw-kk8192-cap)"""
    case = R.OVER_CAP
    weights, _ = R.exact_case(case, "grid", 1)
    path = W.write(str(tmp_path / "over.onnx"), R.graph(case, weights, case["probe"]))
    try:
        with pytest.raises(gpu_api.InferaError, match="8192"):
            gpu_api.load_model("conv_over_cap", path)
    finally:
        try:
            gpu_api.unload_model("conv_over_cap")  # (only there if the load went through)
        except gpu_api.InferaError:
            pass


@pytest.mark.parametrize("case", R.NEIGHBOURS_NCHW, ids=lambda c: c["id"])
def test_neighbouring_nchw_kernels(gpu_api, tmp_path, case):
    run_exact(gpu_api, tmp_path, case)


@pytest.mark.parametrize("case", R.AVG_NCHW, ids=lambda c: c["id"])
def test_nchw_average_pools_divide_the_exact_sum(gpu_api, tmp_path, case):
    run_exact(gpu_api, tmp_path, case, want_of=lambda c, w, x, kind: R.avg_exact(c, w, x))


@pytest.mark.parametrize("layout", ["NC/4HW4", "NCHW"])
@pytest.mark.parametrize("case", R.PER_CHANNEL_EXACT, ids=lambda c: c["id"])
def test_per_channel_operators_exact(gpu_api, tmp_path, case, layout):
    run_exact(gpu_api, tmp_path, case if layout == case["layout"] else R.as_nchw(case))


def identity_weights(case):
    """generic weights for the steps the two plans serve with the same kernel; selection weights (one +-2^e per feature, no bias: one term per sum,
    the same f32 from any kernel) for the convolutions they serve with different ones -- the stem, the gate's 1x1 layer"""
    weights = R.generic_weights(case)
    rng = np.random.default_rng(5)
    sh = R.shapes(case)
    for i, o in enumerate(case["ops"]):
        if o["op"] == "conv" and case["expect"][i] != "normal":
            weights[i] = (R._selection_conv(rng, o["M"], sh[o["src"] if o.get("src") is not None else i][0] // o["g"], o["k"], o["g"]), None)
    return weights


@pytest.mark.parametrize("case", R.GENERIC_CQ_GROUPED + R.PER_CHANNEL_EXACT + R.PER_CHANNEL, ids=lambda c: c["id"])
def test_the_nchw_plan_of_the_same_graph_gives_the_same_bits(gpu_api, tmp_path, case):
    weights = identity_weights(case)
    shape = R.shapes(case)[-1]
    for name, x in R.generic_inputs(case, 3).items():
        quads, plan_q, _ = serve(gpu_api, tmp_path, case, weights, {3: x}, probe="A")
        plain, plan_p, _ = serve(gpu_api, tmp_path, case, weights, {3: x}, probe="")
        check_plan(case, plan_q)
        check_plan(R.as_nchw(case), plan_p)
        a, b = quads[3].reshape(3, *shape), R.through_probe(plain[3].reshape(3, *shape), "A")  # (probe A hands a -0.0 on as +0.0)
        assert np.isfinite(b).all() and np.count_nonzero(b) > b.size // 4
        assert not where_wrong(a, b), (case["id"], name, where_wrong(a, b))


def _figures(case, plan, name, got, ref, bound, theirs):
    err, err_o = np.abs(got - ref), np.abs(theirs - ref)
    ratio = R.rms(err) / R.rms(err_o) if R.rms(err_o) > 0 else (np.inf if R.rms(err) > 0 else 0.0)
    print(f"RATIO {case['id']} {case['layout']} {name}: exec {plan['exec']}: worst error / bound = {(err / bound).max():.4f}, oracle's worst / bound = "
          f"{(err_o / bound).max():.4f}, RMS error / the oracle's = {ratio:.3f}")
    return err, err_o, ratio


def _oracle(tmp_path, case, weights, x, shape):
    from oracle import oracle

    return oracle.Model(W.write(str(tmp_path / "plain.onnx"), R.graph(case, weights, ""))).predict_blob(x.tobytes()).reshape(shape).astype(np.float64)


@pytest.mark.parametrize("case", R.GENERIC_G, ids=lambda c: c["id"])
def test_generic_data_within_the_float64_bound(gpu_api, built, tmp_path, case):
    weights = R.generic_weights(case)
    for name, x in R.generic_inputs(case, 3).items():
        ref, bound = R.error_bound(case, weights, x)
        out, plan, _ = serve(gpu_api, tmp_path, case, weights, {3: x, 1: x[1:2]}, probe=case["probe"])
        check_plan(case, plan)
        got = out[3].reshape(ref.shape)
        alone = out[1].reshape(1, *ref.shape[1:])
        assert not where_wrong(alone, got[1:2]), ("a row alone", name, where_wrong(alone, got[1:2]))
        err, err_o, ratio = _figures(case, plan, name, got.astype(np.float64), ref, bound, _oracle(tmp_path, case, weights, x, ref.shape))
        assert (err <= bound).all(), (name, float((err / bound).max()))
        assert R.rms(err) <= 2 * R.rms(err_o), (name, ratio)


@pytest.mark.parametrize("layout", ["NC/4HW4", "NCHW"])
@pytest.mark.parametrize("case", R.PER_CHANNEL, ids=lambda c: c["id"])
def test_per_channel_operators_on_generic_data(gpu_api, built, tmp_path, case, layout):
    """gate and bn within their derived terms (conv_ref.error_bound); LRN within the parity bar 1e-4 |ref| + 1e-6 of float64 -- the device's powf has no
    documented accuracy to derive a bound from.  LRN reads a selection stem (+-2^e x, exact): the bar is held by lrn_kernel alone, not shared with the
    cancelling sums of a stem in front of it."""
    is_lrn = case["ops"][-1]["op"] == "lrn"
    weights = identity_weights(case) if is_lrn else R.generic_weights(case)
    case = case if layout == case["layout"] else R.as_nchw(case)
    for name, x in R.generic_inputs(case, 3).items():
        ref, bound = R.error_bound(case, weights, x)
        out, plan, _ = serve(gpu_api, tmp_path, case, weights, {3: x}, probe=case["probe"])
        check_plan(case, plan)
        got = out[3].reshape(ref.shape).astype(np.float64)
        err, err_o, ratio = _figures(case, plan, name, got, ref, R.lrn_bar(ref) if is_lrn else bound, _oracle(tmp_path, case, weights, x, ref.shape))
        assert (err <= (R.lrn_bar(ref) if is_lrn else bound)).all(), (name, float((err / (R.lrn_bar(ref) if is_lrn else bound)).max()))
