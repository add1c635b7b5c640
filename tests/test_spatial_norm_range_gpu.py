"""The SpatialNorm kernels (hip/spatialnorm.hip) on every launch form and at the value edges, through the C ABI, against float64 at the
parity bar of DESIGN.md section 5, max |got - ref| / (1e-4 |ref| + 1e-6) <= 1 over every element.  The cases are the table of
tests/spatial_norm_cases.py, which tests/test_spatial_norm_cases.py proves to reach all seven instantiations of the fused kernel with one
group per unit (mode 0) and with one quad plane per unit (mode 1), both sides of every boundary between them, the element-by-element form
with several quads per lane, [N,C,1,1] tensors, and in the general plan the second step of every loop: the stats kernel's element loop,
groups that straddle quads, and the apply kernel's grid-stride loop by elements and by quads.  The values: a common offset of 0 and of 1000,
magnitudes of 2^40 and 2^-20, a variance comparable to epsilon and one far below it, and groups dominated by one outlier.  Groups that share
a wave, a quad plane or a workgroup must not see each other: changing one group -- by finite values, a NaN, an Inf -- leaves every other
element its bits.

Worst ratio to the bar, measured on an MI355X (2026-10-21); every test passed, no case came near the bar.
  test_every_rung_at_the_parity_bar, by instantiation <L,NV> (offsets 0 and 1000, no activation and SiLU, all row counts):
    mode 0, NCHW:          <8,1> 0.0413  <16,1> 0.0406  <32,1> 0.0708  <64,1> 0.0571  <64,4> 0.0914  <64,16> 0.0872  <256,16> 0.0916
    mode 0, channel quads: <8,1> 0.0368  <64,4> 0.0876  <64,16> 0.0721
    mode 1:                <8,1> 0.0394  <16,1> 0.0473  <32,1> 0.0898  <64,1> 0.0555  <64,4> 0.0692  <64,16> 0.0805  <256,16> 0.1003
    general plan:          E = 16385 0.0854, planes of 4097 0.0582, (12, 4, 10 x 10) 0.0825, 17 x 17 forced 0.0663, and the second step
                           of the apply loop 0.1051 by elements (33 x 255 x 257) and 0.1042 by quads (129 x 256 x 256)
  test_plans_agree_where_both_exist (3 rows): the fused kernel at most 0.0814, the general plan on the same layers at most 0.0874.
  test_value_edges, worst over the fused instantiations / on the general plan: big 0.0875 (mode 1 <256,16>) / 0.0703; small 0.0566 (mode 1
    <256,16>) / 0.0550; eps_rules 0.0368 / 0.0564; outlier 0.0284 (mode 1 <32,1>) / 0.0065.
  ChannelNorm's test_value_edges (tests/test_channel_norm_gpu.py): big 0.1902, small 0.0627, eps_rules 0.0536, outlier 0.1095.
The float32 emulation of tests/spatial_norm_cases.py on a CPU gives 0.004-0.08 for the same kinds of input."""
from __future__ import annotations

import numpy as np
import pytest

from infera_amd import onnx_writer as W
from tests import spatial_norm_cases as SC
from tests.test_spatial_norm_gpu import bar_ratio, check_layouts, gamma_beta, same_bits, serve

pytestmark = pytest.mark.gpu

FUSED, GENERAL = ["spatialnorm_fused"], ["spatialnorm_stats", "spatialnorm_apply"]


@pytest.fixture(scope="module")
def api(built):
    from infera_amd import capi

    assert capi.device_count() >= 1, capi.get_devices()
    return capi


def model_of(k, act=None, eps=1e-5):
    op = "InstanceNormalization" if k.g == k.c else "GroupNormalization"
    return W.spatial_norm_model(k.c, k.g, k.hw, op=op, form="op21", act=act, eps=eps, **SC.LAYOUTS[k.layout])


def check_plan(m, k, plan=None):
    plan = plan or k.plan
    want = FUSED if k.unit is not None and plan == "default" else GENERAL
    assert [s["kernel"] for s in m.plan["spatialnorm"]] == want, m.plan["spatialnorm"]
    check_layouts(m, k.layout)


def tag(k):
    return "general" if k.label is None else "mode %d <%d,%d>" % k.label


# ---- every rung, every loop ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [k.name for k in SC.TABLE])
def test_every_rung_at_the_parity_bar(api, tmp_path, monkeypatch, name):
    """x = offset + U(-1, 1) at offsets 0 and 1000, without an activation and with SiLU, for the case's row counts: the bar over every
    element; a row alone gives the bits it has inside its batch, a second call the same bits.  A group of one element (E = 1) has d = 0:
    y = act(beta[c]) bit for bit."""
    k = SC.BY_NAME[name]
    worst = 0.0
    for act in (None,) if k.light else (None, "Silu"):
        blob, spec = model_of(k, act)
        with serve(api, tmp_path, monkeypatch, blob, k.plan) as m:
            check_plan(m, k)
            assert m.plan["spatialnorm"][-1]["act"] == ("Swish" if act else "")
            for offset in (0.0, 1000.0):
                spec["offset"] = offset
                for n in k.rows:
                    x = W.spatial_norm_inputs(spec, n, seed=100 + n)
                    want = W.decoder_reference(spec, x).reshape(n, -1)
                    got = m(x)
                    ratio = bar_ratio(got, want)
                    worst = max(worst, ratio)
                    assert ratio <= 1.0, (act, offset, n, ratio)
                    if not k.light:
                        assert same_bits(m(x), got), "two runs of the same call differ"
                    if n > 1:
                        assert same_bits(m(x[n - 2:n - 1]), got[n - 2]), "a row alone differs from the row in its batch"
    print(f"\n{name} [{tag(k)}]: worst max |err| / (rtol |ref| + atol) = {worst:.4f}")
    if k.e == 1:
        x = W.spatial_norm_inputs(dict(spec, offset=1000.0), 3, seed=7)
        for act in (None, "Relu"):
            blob, spec = model_of(k, act)
            _, beta = gamma_beta(spec)
            with serve(api, tmp_path, monkeypatch, blob, k.plan) as m:
                check_plan(m, k)
                assert same_bits(m(x), np.broadcast_to(np.maximum(beta, 0) if act else beta, (3, k.c)))


# ---- the value edges -----------------------------------------------------------------------------------------------------------------
VALUES = [("big", 0.0), ("small", 0.0), ("eps_rules", 0.0), ("outlier", 0.0), ("outlier", 1000.0)]


@pytest.mark.parametrize("kind", list(SC.VALUE_KINDS))
def test_value_edges(api, tmp_path, monkeypatch, kind):
    """One case per rung and mode and the general cases, with 2^40 U(-1, 1), with 2^-20 U(-1, 1) under epsilon = 1e-12 (the variance is
    comparable to epsilon), with 2^-10 U(-1, 1) (epsilon is 30 times the variance) and with one element of every group at 1e4, also on a
    common offset of 1000: the same bar against the same float64 reference, with the case's epsilon."""
    worst = {}
    for name in SC.EDGE_CASES:
        k = SC.BY_NAME[name]
        blob, spec = model_of(k, eps=SC.VALUE_KINDS[kind][1])
        with serve(api, tmp_path, monkeypatch, blob, k.plan) as m:
            check_plan(m, k)
            for offset in [o for kd, o in VALUES if kd == kind]:
                spec["offset"] = offset
                for n in k.rows[:2]:
                    x, _ = SC.value_inputs(spec, n, kind, seed=200 + n)  # (asserts that the model carries the kind's epsilon)
                    ratio = bar_ratio(m(x), W.decoder_reference(spec, x).reshape(n, -1))
                    worst[tag(k)] = max(worst.get(tag(k), 0.0), ratio)
                    assert ratio <= 1.0, (name, offset, n, ratio)
    print(f"\n{kind}: worst max |err| / (rtol |ref| + atol) = " + ", ".join(f"{t} {r:.4f}" for t, r in worst.items()))


# ---- groups next to each other -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [k.name for k in SC.NEIGHBOUR_CASES])
def test_groups_do_not_see_each_other(api, tmp_path, monkeypatch, name):
    """Several groups share a wave (L < 64), a quad plane (mode 1) or the quads of a plane (the general plan).  One group of one row is
    redrawn and shifted by 512: every element outside it, in its row and in the others, keeps its bits, and the group still meets the bar.
    On NCHW tensors (the identity convolution in front of a channel-quad layer multiplies a non-finite value by zero) the same with one
    NaN and with one +Inf in the group: the group comes out all NaN, everything else keeps its bits."""
    k = next(c for c in SC.NEIGHBOUR_CASES if c.name == name)
    n, cg = 3, k.c // k.g
    blob, spec = model_of(k)
    x = W.spatial_norm_inputs(spec, n, seed=11)
    with serve(api, tmp_path, monkeypatch, blob, k.plan) as m:
        check_plan(m, k)
        clean = m(x).reshape(x.shape)
        for group in sorted({0, k.g // 2, k.g - 1}):
            inside = np.zeros(x.shape, bool)
            inside[1, group * cg:(group + 1) * cg] = True
            other = x.copy()
            other[inside] = 512.0 + np.random.default_rng(12 + group).uniform(-1, 1, int(inside.sum())).astype(np.float32)
            got = m(other).reshape(x.shape)
            assert same_bits(got[~inside], clean[~inside]), (group, "finite")
            want = W.decoder_reference(spec, other).reshape(x.shape)
            ratio = bar_ratio(got[inside], want[inside])
            assert ratio <= 1.0, (group, ratio)
            if k.layout != SC.NCHW:
                continue
            for bad in (np.nan, np.inf):
                other = x.copy()
                other[(1, group * cg + cg // 2) + tuple(h // 2 for h in k.hw)] = bad
                got = m(other).reshape(x.shape)
                assert same_bits(got[~inside], clean[~inside]), (group, bad)
                assert np.isnan(got[inside]).all(), (group, bad)


# ---- the two plans -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [k.name for k in SC.TABLE if k.fused])
def test_plans_agree_where_both_exist(api, tmp_path, monkeypatch, name):
    """A layer with a fused form also runs on the general plan (INFERA_SPATIALNORM_FUSED=0).  The two divide in different places (d / den
    against d * inv), so their bits may differ; each meets the bar on its own."""
    k = SC.BY_NAME[name]
    blob, spec = model_of(k)
    worst = {}
    for plan in ("default", "general"):
        with serve(api, tmp_path, monkeypatch, blob, plan) as m:
            check_plan(m, k, plan)
            for offset in (0.0, 1000.0):
                spec["offset"] = offset
                n = k.rows[1]
                x = W.spatial_norm_inputs(spec, n, seed=300 + n)
                ratio = bar_ratio(m(x), W.decoder_reference(spec, x).reshape(n, -1))
                worst[plan] = max(worst.get(plan, 0.0), ratio)
                assert ratio <= 1.0, (plan, offset, ratio)
    print(f"\n{name} [{tag(k)}]: fused {worst['default']:.4f}, general {worst['general']:.4f}")
