"""What tests/test_spatial_norm_range_gpu.py runs, checked without a GPU: the case table reaches every launch form it claims to reach,
and the inputs at the value edges can meet the parity bar in float32 arithmetic of the documented order."""
from __future__ import annotations

import numpy as np
import pytest

from infera_amd import onnx_writer as W
from tests import spatial_norm_cases as SC

# every (mode, L, NV) the table must reach, by layout
CLAIMED = {
    SC.NCHW: {(0, 8, 1), (0, 16, 1), (0, 32, 1), (0, 64, 1), (0, 64, 4), (0, 64, 16), (0, 256, 16)},
    SC.CQ: {(1, 8, 1), (1, 16, 1), (1, 32, 1), (1, 64, 1), (1, 64, 4), (1, 64, 16), (1, 256, 16), (0, 8, 1), (0, 64, 4), (0, 64, 16)},
}


def test_the_restated_ladder():
    assert [SC.rung_of(u) for u in (1, 32, 33, 64, 65, 128, 129, 256, 257, 1024, 1025, 4096, 4097, 16384)] == [
        (8, 1), (8, 1), (16, 1), (16, 1), (32, 1), (32, 1), (64, 1), (64, 1), (64, 4), (64, 4), (64, 16), (64, 16), (256, 16), (256, 16)]
    for top, l, nv in SC.LADDER:
        assert 4 * l * nv >= top, "a rung holds its largest unit in registers"
    assert SC.unit_of(8, 8, 35, False) == (0, 35) and SC.unit_of(8, 8, 35, True) == (1, 140) and SC.unit_of(8, 4, 35, True) == (1, 140)
    assert SC.unit_of(8, 2, 35, True) == (0, 140) and SC.unit_of(12, 4, 9, True) is None and SC.unit_of(12, 4, 1, True) == (0, 3)
    assert SC.unit_of(4, 1, 72 * 72, False) is None and SC.unit_of(4, 4, 4097, True) is None and SC.unit_of(4, 4, 4096, True) == (1, 16384)


def test_the_table_reaches_every_form_it_claims():
    reached = {layout: {k.label for k in SC.TABLE if k.layout == layout and k.label} for layout in SC.LAYOUTS}
    for layout, want in CLAIMED.items():
        assert want <= reached[layout], (layout, sorted(want - reached[layout]))
    print("\nreached:", {layout: sorted(v) for layout, v in reached.items()})
    # every boundary of the ladder from both sides, in mode 0 (NCHW: U and U + 1) and in mode 1 (U = 4 S: the nearest planes)
    units = {mode: {k.unit[1] for k in SC.TABLE if k.label and k.label[0] == mode} for mode in (0, 1)}
    for top in SC.BOUNDARIES[:-1]:
        assert {top, top + 1} <= units[0], top
        assert {top, top + 4} <= units[1], top
    assert SC.FUSED_MAX in units[0] and SC.FUSED_MAX in units[1]
    beyond = {(k.layout, k.unit) for k in SC.TABLE if (k.c, k.g, k.hw) in ((3, 3, (16385,)), (4, 4, (4097,)))}
    assert beyond == {(SC.NCHW, None), (SC.CQ, None)}
    # the element-by-element fused kernel with more than one quad per lane
    assert any(k.label and k.label[2] > 1 and k.unit[1] % 4 for k in SC.TABLE)
    # idle unit slots in the last workgroup: 3 units per row do not fill 256 / L slots for 1 row at any L < 256
    assert all((n * 3) % (256 // k.label[1]) for k in SC.TABLE if k.layout == SC.NCHW and k.label and k.label[1] < 256 and k.c == 3 for n in (1, 3))


def test_what_plans_general_does_so_by_the_unit_rule():
    for k in SC.TABLE:
        assert k.fused == (k.unit is not None and k.plan == "default"), k
        assert k.c % k.g == 0 and (k.layout == SC.NCHW or k.c % 4 == 0), k
        if not k.light:
            floats = k.unit[1] if k.unit else max(k.e, 4 * k.s if k.layout == SC.CQ else 0)  # of a work unit, or of a group / its planes
            assert k.rows == ((1, 3, 70) if floats <= 4100 else (1, 3)), k
    general = {k.name: k for k in SC.TABLE if not k.fused}
    assert sorted(general) == sorted(["nchw_c3_g3_16385", "cq_c4_g4_4097", "cq_c12_g4_10x10", "nchw_c3_g3_17x17_general", "nchw_c1_g1_255x257",
                                      "nchw_c1_g1_256x256"])
    # the loops the general cases are there for
    k = general["cq_c12_g4_10x10"]
    assert (k.c // k.g) % 4 and k.s > 1 and k.e > 256, "non-contiguous groups, the element loop of the stats kernel twice"
    k = general["nchw_c3_g3_17x17_general"]
    assert k.e % 4 and k.e > 256
    k = general["nchw_c1_g1_255x257"]
    assert k.e % 4 and k.rows[0] * k.e > 8192 * 256, "the element form of the apply kernel takes a second step"
    k = general["nchw_c1_g1_256x256"]
    assert k.e % 4 == 0 and k.rows[0] * k.e // 4 > 8192 * 256, "the quad form of the apply kernel takes a second step"
    for names in (SC.EDGE_CASES, [k.name for k in SC.NEIGHBOUR_CASES[1:]]):
        assert set(names) <= set(SC.BY_NAME)
    edge = {SC.BY_NAME[n].label for n in SC.EDGE_CASES}
    assert {(m, l, nv) for m in (0, 1) for l, nv in SC.RUNGS} <= edge and None in edge


def test_value_inputs_are_what_they_say():
    for kind, (scale, eps) in SC.VALUE_KINDS.items():
        blob, spec = W.spatial_norm_model(8, 4, (5, 7), op="GroupNormalization", eps=eps)
        spec["offset"] = 1000.0 if kind == "outlier" else 0.0
        x, got_eps = SC.value_inputs(spec, 3, kind, seed=1)
        assert x.dtype == np.float32 and x.shape == (3, 8, 5, 7) and got_eps == eps
        g = x.reshape(3 * 4, 70).astype(np.float64) - spec["offset"]
        if kind == "outlier":
            assert ((g == SC.OUTLIER).sum(axis=1) == 1).all()
        else:
            assert np.abs(g).max() <= scale and np.abs(g).max() > scale / 2
            assert 0.2 * scale ** 2 < g.var(axis=1).mean() < 0.45 * scale ** 2


FEASIBLE_E = [19, 35, 257, 1025, 4097, 16384, 65535]
FEASIBLE_KINDS = [("plain", 0.0), ("plain", 1000.0), ("big", 0.0), ("small", 0.0), ("eps_rules", 0.0), ("outlier", 0.0), ("outlier", 1000.0)]


@pytest.mark.parametrize("general", [False, True], ids=["fused", "general"])
@pytest.mark.parametrize("kind,offset", FEASIBLE_KINDS)
def test_float32_arithmetic_of_the_documented_order_meets_a_quarter_of_the_bar(kind, offset, general):
    """emulate_f32 against float64 stays at or below 0.25 of |err| / (1e-4 |ref| + 1e-6) for every kind of input the GPU tests draw, at
    group sizes from 19 to 65535: the bar of 1 leaves the device's own summation order a factor of four."""
    worst = 0.0
    for e in FEASIBLE_E:
        rng = np.random.default_rng(e)
        gamma, beta = rng.uniform(0.5, 1.5, e).astype(np.float32), rng.uniform(-0.5, 0.5, e).astype(np.float32)
        n = 6 if e < 5000 else 2
        if kind == "plain":
            x, eps = (offset + rng.uniform(-1, 1, (n, e))).astype(np.float32), 1e-5
        else:
            x, eps = SC.value_groups(n, e, kind, seed=e, offset=offset), SC.VALUE_KINDS[kind][1]
        eps = float(np.float32(eps))
        ratio = SC.bar_ratio(SC.emulate_f32(x, gamma, beta, eps, general), SC.reference_f64(x, gamma, beta, eps))
        print(f"{kind} offset={offset:g} E={e} {'general' if general else 'fused'}: {ratio:.4f}")
        worst = max(worst, ratio)
        assert ratio <= 0.25, (e, ratio)
    assert worst > 0.0
