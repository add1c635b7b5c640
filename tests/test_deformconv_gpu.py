"""DeformConv on the GPU (INTEGRATION.md 2.6 "Deformable convolutions"), through predict_from_blob, against the float64 loop of
tests/deformconv_ref.py.  Every case is the smallest shape at which something specific can go wrong, and runs twice:
  exact    X whole multiples of 4, weights and bias whole numbers, offsets multiples of 0.5, mask in {0, 0.5, 1}: every bilinear weight is a multiple
           of 0.25 and every product and partial sum is exact (the reference's magnitude stays below 2^23), so the result equals the reference
           bit for bit in any summation order.
  normal   normal X and W, offsets on a 2^-8 grid (coordinates and bilinear weights exact in f32).  What rounds: five operations on a sample, the
           K-term fma chain, the bias add: |got - ref| <= (K + 8) * 2^-24 * mag per element.  The worst ratio of each case is printed;
           profiles/deformconv_error_ratios.txt records the table.
The edge-value case was run only after tests/native/deformconv_index (the same coordinate function under host sanitizers) was clean."""
from __future__ import annotations

import numpy as np
import pytest

from infera_amd import onnx_writer as W

import deformconv_ref as R

pytestmark = pytest.mark.gpu
CQ, NCHW = "NC/4HW4", "NCHW"

CASES = {  # id: (C, M, (H, W), (kh, kw), attrs, mask, exec)
    "degenerate": (1, 1, (1, 1), (1, 1), {}, False, "deformconv_mfma"),
    "channel_and_m_straddle": (3, 5, (5, 6), (3, 3), dict(pads=[1, 1, 1, 1]), True, "deformconv_mfma"),
    "second_m_tile": (8, 33, (7, 7), (3, 3), dict(pads=[1, 1, 1, 1]), False, "deformconv_mfma"),
    "position_tail": (4, 4, (3, 11), (1, 1), {}, True, "deformconv_mfma"),  # (OH * OW = 33)
    "odd_tail_chunk": (13, 24, (4, 5), (3, 3), dict(pads=[1, 1, 1, 1]), True, "deformconv_mfma"),  # (K = 117: an odd last k-pair too)
    "five_m_tiles": (4, 132, (3, 4), (1, 1), {}, False, "deformconv_mfma"),  # (two tiles per wave, the last wave's second one absent)
    "nine_m_tiles": (4, 264, (2, 3), (1, 1), {}, False, "deformconv_mfma"),  # (four tiles per wave)
    "seventeen_m_tiles": (2, 520, (2, 2), (1, 1), {}, False, "deformconv_mfma"),  # (a second work group along M)
    "offset_group_2": (8, 6, (5, 5), (3, 3), dict(pads=[1, 1, 1, 1], offset_group=2), True, "deformconv_mfma"),
    "offset_group_c": (6, 4, (4, 5), (2, 2), dict(offset_group=6), False, "deformconv_mfma"),
    "geometry": (5, 7, (9, 8), (2, 3), dict(strides=[2, 2], dilations=[2, 2], pads=[1, 0, 2, 1]), True, "deformconv_mfma"),
    "group_2": (6, 4, (5, 5), (3, 3), dict(pads=[1, 1, 1, 1], group=2, offset_group=3), True, "deformconv_generic"),
    "taps_above_the_cap": (2, 3, (6, 11), (5, 10), dict(pads=[2, 4, 2, 5]), False, "deformconv_generic"),
}


@pytest.fixture(scope="module")
def api(built):
    from infera_amd import capi

    assert capi.device_count() >= 1, capi.get_devices()
    return capi


def run(api, tmp_path, blob, *inputs):
    """one load, one call: the inputs' rows side by side, as a multi-input model takes them"""
    api.load_model("dcn", W.write(str(tmp_path / "dcn.onnx"), blob))
    try:
        rows = np.ascontiguousarray(np.hstack([np.asarray(a, np.float32).reshape(len(a), -1) for a in inputs]))
        return api.get_plan("dcn"), api.predict_from_blob("dcn", rows.tobytes()).reshape(len(rows), -1)
    finally:
        api.unload_model("dcn")


def draw(case, exact, n=3, seed=5):
    """-> (the model, its inputs, the keyword arguments of the reference)"""
    C, M, hw, k, attrs, mask, _ = CASES[case]
    rng = np.random.default_rng(seed)
    g, og = attrs.get("group", 1), attrs.get("offset_group", 1)
    OH, OW = W.deform_conv_out_hw(hw, k, attrs.get("strides", (1, 1)), attrs.get("pads", (0, 0, 0, 0)), attrs.get("dilations", (1, 1)))
    shapes = dict(x=(n, C, *hw), w=(M, C // g, *k), off=(n, og * k[0] * k[1] * 2, OH, OW), mask=(n, og * k[0] * k[1], OH, OW))
    if exact:
        x, w, b = 4.0 * rng.integers(-4, 5, shapes["x"]), rng.integers(-4, 5, shapes["w"]), rng.integers(-4, 5, M)
        off, mk = rng.integers(-6, 7, shapes["off"]) / 2.0, rng.integers(0, 3, shapes["mask"]) / 2.0
    else:
        x, w, b = rng.normal(size=shapes["x"]), rng.normal(size=shapes["w"]) / np.sqrt(C // g * k[0] * k[1]), rng.normal(size=M)
        off, mk = rng.integers(-768, 769, shapes["off"]) / 256.0, rng.uniform(0, 1, shapes["mask"])
    x, w, b, off, mk = (a.astype(np.float32) for a in (x, w, b, off, mk))
    blob = W.deform_conv_layer(w, b, hw, mask=mask, **attrs)
    return blob, [x, off] + ([mk] if mask else []), dict(x=x, w=w, off=off, b=b, mask=mk if mask else None, **{kk: v for kk, v in attrs.items() if kk != "group"}, group=g)


def reference(kw):
    return R.deform_conv64(kw["x"], kw["w"], kw["off"], kw["b"], kw["mask"], kw.get("strides", (1, 1)), kw.get("pads", (0, 0, 0, 0)), kw.get("dilations", (1, 1)),
                           kw["group"], kw.get("offset_group", 1))


@pytest.mark.parametrize("case", list(CASES))
def test_exact_data_equals_the_reference_bit_for_bit(api, tmp_path, case):
    blob, inputs, kw = draw(case, exact=True)
    plan, got = run(api, tmp_path, blob, *inputs)
    assert plan["deformconv"][0]["exec"] == CASES[case][6]
    want, mag = reference(kw)
    assert mag.max() < 2.0 ** 23
    assert np.array_equal(got.astype(np.float64), want.reshape(len(want), -1)), float(np.abs(got - want.reshape(len(want), -1)).max())


@pytest.mark.parametrize("case", list(CASES))
def test_normal_data_within_the_rounding_bound(api, tmp_path, case):
    blob, inputs, kw = draw(case, exact=False)
    plan, got = run(api, tmp_path, blob, *inputs)
    assert plan["deformconv"][0]["exec"] == CASES[case][6]
    want, mag = reference(kw)
    K = kw["w"][0].size
    ratio = float((np.abs(got - want.reshape(len(want), -1)) / ((K + 8) * 2.0 ** -24 * mag.reshape(len(want), -1))).max())
    print(f"deformconv error ratio: {case:24s} K {K:4d}  worst |got - ref| / bound = {ratio:.3f}")
    assert ratio <= 1.0, ratio


def test_a_row_alone_has_the_bits_it_has_in_a_batch_of_five(api, tmp_path):
    blob, inputs, _ = draw("odd_tail_chunk", exact=False, n=5)
    _, five = run(api, tmp_path, blob, *inputs)
    for r in (0, 4):
        _, one = run(api, tmp_path, blob, *[a[r:r + 1] for a in inputs])
        assert np.array_equal(one[0].view(np.uint32), five[r].view(np.uint32))


def test_the_generic_kernel_agrees_with_the_mfma_form(api, tmp_path, monkeypatch):
    blob, inputs, _ = draw("geometry", exact=False)
    plan, mfma = run(api, tmp_path, blob, *inputs)
    monkeypatch.setenv("INFERA_DEFORMCONV_MFMA", "0")
    plan0, generic = run(api, tmp_path, blob, *inputs)
    assert (plan["deformconv"][0]["exec"], plan0["deformconv"][0]["exec"]) == ("deformconv_mfma", "deformconv_generic")
    assert np.all(np.abs(generic - mfma) <= 1e-4 * np.abs(mfma) + 1e-6), float(np.abs(generic - mfma).max())  # (the parity bar of the network tests)


@pytest.mark.parametrize("k,layout,og", [(2, CQ, 1), (2, CQ, 4), (3, NCHW, 1)])  # (og = 4: two channels per offset group, inside a quad)
def test_a_dcn_block_end_to_end(api, tmp_path, k, layout, og):
    blob, w = W.dcn_block(k=k, offset_group=og, offset_scale=4.0)
    x = np.random.default_rng(31).uniform(-1, 1, size=(3, 3, 6, 7)).astype(np.float32)
    plan, got = run(api, tmp_path, blob, x)
    d = plan["deformconv"][0]
    assert plan["activation_layout"] == layout and (d["exec"], d["in_layout"], d["out_layout"], d["offset_layout"]) == ("deformconv_mfma", layout, layout, layout)
    want = R.dcn_block64(w, x, k, og)
    assert np.all(np.abs(got - want) <= 1e-4 * np.abs(want) + 1e-6), float(np.abs(got - want).max())


def test_edge_values_follow_the_contract(api, tmp_path):
    """offsets of +-inf, NaN, +-1e30, exactly -1 (the coordinate of tap 0 at the first position), exactly H and H - 1 + 2^-20: a NaN offset gives NaN at
    exactly the outputs that read it; every other output equals the reference, to the bound of the normal run"""
    C, M, (H, Wd) = 3, 4, (5, 6)
    rng = np.random.default_rng(37)
    x, w, b = rng.uniform(0.5, 1.5, (2, C, H, Wd)).astype(np.float32), rng.normal(size=(M, C, 1, 1)).astype(np.float32), rng.normal(size=M).astype(np.float32)
    edge = np.array([np.inf, -np.inf, np.nan, 1e30, -1e30, -1.0, H, H - 1 + 2.0 ** -20, 0.25, -0.5], np.float32)
    off = rng.choice(edge, size=(2, 2, H, Wd)).astype(np.float32)
    off[0, :, 0, 0] = -1.0, float(Wd)  # (position (0, 0): its coordinates are the offsets themselves)
    off[0, :, 0, 1] = H - 1 + 2.0 ** -20, np.nan
    _, got = run(api, tmp_path, W.deform_conv_layer(w, b, (H, Wd)), x, off)
    want, mag = R.deform_conv64(x, w, off, b)
    want, mag, got = want.reshape(2, M, -1), mag.reshape(2, M, -1), got.reshape(2, M, -1)
    nan = np.isnan(off).any(1).reshape(2, 1, -1).repeat(M, 1)
    assert nan.any() and (~nan).any() and np.array_equal(np.isnan(got), nan) and np.array_equal(np.isnan(want), nan)
    assert np.all(np.abs(got - want)[~nan] <= (C + 8) * 2.0 ** -24 * mag[~nan])
    assert np.array_equal(got[0, :, 0], b)  # (coordinates (-1, W): nothing is read, the bias alone)
