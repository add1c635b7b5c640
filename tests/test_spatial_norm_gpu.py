"""InstanceNormalization and GroupNormalization on the GPU, through the C ABI.  Every layout case of the
SpatialNorm kernels -- NCHW tensors and channel-quad planes, the fused one-pass kernel and the SpatialStats + SpatialNorm pair -- against the
float64 reference at the parity bar of DESIGN.md section 5 (every element, at a common input offset of 0 and of 1000), the cases whose
result is known bit for bit, the bit identities (a row alone and in its batch, the host path and the device-resident entry, two runs, the
operator and the exporter's spelling, rows next to a NaN row), and the writer's two whole models."""
from __future__ import annotations

import numpy as np
import pytest

from infera_amd import onnx_writer as W

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 1e-6
# identity 1x1 layers around the layer under test put it on channel-quad tensors (the model's own input and a served [C,H,W] result are NCHW)
LAYOUTS = {"nchw_in_nchw_out": dict(pre=False, post=False), "cq_in_cq_out": dict(pre=True, post=True)}
PLANS = {"default": None, "general": "0"}  # INFERA_SPATIALNORM_FUSED
FUSED_MAX = 16384
# (C, G, spatial extents)
CASES = {
    "inorm_8x5x7": (8, 8, (5, 7)),         # E = 35: scalar tails, units not 16-byte aligned in NCHW; one quad plane = 4 groups in channel quads
    "cg2_8x5x7": (8, 4, (5, 7)),           # two groups per quad plane
    "cg4_8x5x7": (8, 2, (5, 7)),           # a contiguous whole-quad group
    "cg3_12x3x3": (12, 4, (3, 3)),         # groups straddle quads: the general plan in channel quads, fused in NCHW
    "g1_32x16x16": (32, 1, (16, 16)),      # E = 8,192: the whole-workgroup form with the LDS join
    "big_4x72x72": (4, 1, (72, 72)),       # E = 20,736 > the fused cap: the general plan in both layouts
    "inorm_1d_8x19": (8, 8, (19,)),        # [N, C, L]
}


@pytest.fixture(scope="module")
def api(built):
    from infera_amd import capi

    assert capi.device_count() >= 1, capi.get_devices()
    return capi


class Served:
    def __init__(self, api, tmp_path, blob, name="sn"):
        self.api, self.name = api, name
        api.load_model(name, W.write(str(tmp_path / f"{name}.onnx"), blob))
        self.plan = api.get_plan(name)

    def __call__(self, x):
        x = np.ascontiguousarray(x, np.float32)
        return self.api.predict_from_blob(self.name, x.tobytes()).reshape(len(x), -1)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.api.unload_model(self.name)


def serve(api, tmp_path, monkeypatch, blob, plan="default", name="sn"):
    if PLANS[plan] is None:
        monkeypatch.delenv("INFERA_SPATIALNORM_FUSED", raising=False)
    else:
        monkeypatch.setenv("INFERA_SPATIALNORM_FUSED", PLANS[plan])  # (read when a model is loaded)
    return Served(api, tmp_path, blob, name)


def same_bits(got, want):
    got, want = np.ascontiguousarray(got, np.float32).reshape(-1), np.ascontiguousarray(want, np.float32).reshape(-1)
    return got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def rows_of(case):
    return (1, 3) if case == "big_4x72x72" else (1, 3, 70)


def model_of(case, layout, act=None, form="op21", **kw):
    c, g, hw = CASES[case]
    op = "InstanceNormalization" if g == c and form == "op21" else "GroupNormalization"
    return W.spatial_norm_model(c, g, hw, op=op, form=form, act=act, **LAYOUTS[layout], **kw)


def expected_kernels(case, layout, plan):
    c, g, hw = CASES[case]
    s, cg = int(np.prod(hw)), c // g
    if layout == "cq_in_cq_out" and cg % 4 != 0:
        fused = cg in (1, 2) and 4 * s <= FUSED_MAX
    else:
        fused = cg * s <= FUSED_MAX
    return ["spatialnorm_fused"] if fused and plan == "default" else ["spatialnorm_stats", "spatialnorm_apply"]


def check_layouts(m, layout):
    want = "NC/4HW4" if layout == "cq_in_cq_out" else "NCHW"
    assert all(k["in_layout"] == want and k["out_layout"] == want for k in m.plan["spatialnorm"]), m.plan["spatialnorm"]


def bar_ratio(got, want):
    return float((np.abs(got.reshape(want.shape) - want) / (RTOL * np.abs(want) + ATOL)).max())


# ---- the parity bar ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan", list(PLANS))
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("case", list(CASES))
def test_parity_bar_at_offsets_0_and_1000(api, tmp_path, monkeypatch, case, layout, plan):
    """max |got - ref| / (1e-4 |ref| + 1e-6) <= 1 against float64 over every element, with x = offset + U(-1, 1), without an activation and
    with SiLU, for 1, 3 and 70 rows; a row alone gives the bits it has inside its batch, and a second run of the same call the same bits."""
    for act in (None, "Silu"):
        blob, spec = model_of(case, layout, act)
        with serve(api, tmp_path, monkeypatch, blob, plan) as m:
            assert [k["kernel"] for k in m.plan["spatialnorm"]] == expected_kernels(case, layout, plan), m.plan["spatialnorm"]
            assert m.plan["spatialnorm"][-1]["act"] == ("Swish" if act else "")
            check_layouts(m, layout)
            for offset in (0.0, 1000.0):
                spec["offset"] = offset
                for n in rows_of(case):
                    x = W.spatial_norm_inputs(spec, n, seed=100 + n)
                    want = W.decoder_reference(spec, x).reshape(n, -1)
                    got = m(x)
                    ratio = bar_ratio(got, want)
                    print(f"{case} {layout} {plan} act={act} offset={offset:g} rows={n}: max |err| / (rtol |ref| + atol) = {ratio:.4f}")
                    assert ratio <= 1.0, (act, offset, n, ratio)
                    assert same_bits(m(x), got), "two runs of the same call differ"
                    if n > 1:
                        assert same_bits(m(x[n - 2:n - 1]), got[n - 2]), "a row alone differs from the row in its batch"


# ---- results known bit for bit -----------------------------------------------------------------------------------------------------
def gamma_beta(spec):
    p = next(p for op, out, ins, p in spec["layers"] if out == "norm")
    return p["gamma"].astype(np.float32), p["beta"].astype(np.float32)


def per_element(v, c, hw):
    """[C] -> [1, C, *hw]"""
    return np.broadcast_to(np.asarray(v).reshape((1, c) + (1,) * len(hw)), (1, c) + tuple(hw))


@pytest.mark.parametrize("plan", list(PLANS))
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("case", list(CASES))
def test_constant_groups_give_the_activated_beta(api, tmp_path, monkeypatch, case, layout, plan):
    """A group whose elements are all equal has d = 0, so y = act(beta[c]) exactly -- also the group that holds 1000.25."""
    c, g, hw = CASES[case]
    n = 3
    vals = np.random.default_rng(3).integers(-64, 65, size=(n, g)).astype(np.float32) / 4
    vals[1, g // 2] = 1000.25
    x = np.broadcast_to(np.repeat(vals, c // g, axis=1).reshape((n, c) + (1,) * len(hw)), (n, c) + tuple(hw))
    for act in (None, "Relu"):
        blob, spec = model_of(case, layout, act)
        _, beta = gamma_beta(spec)
        want = per_element(np.maximum(beta, 0) if act else beta, c, hw)
        with serve(api, tmp_path, monkeypatch, blob, plan) as m:
            got = m(x)
        assert same_bits(got, np.broadcast_to(want, (n, c) + tuple(hw))), (act, float(np.abs(got.reshape(x.shape) - want).max()))


HALF_CASES = {"cg1_8x4x6": (8, 8, (4, 6)), "cg2_8x5x7": CASES["cg2_8x5x7"], "cg4_8x5x7": CASES["cg4_8x5x7"], "cg3_12x4x4": (12, 4, (4, 4)),
              "g1_32x16x16": CASES["g1_32x16x16"], "big_4x72x72": CASES["big_4x72x72"]}


@pytest.mark.parametrize("plan", list(PLANS))
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("case", list(HALF_CASES))
def test_half_plus_one_half_minus_one(api, tmp_path, monkeypatch, case, layout, plan):
    """A group that is half +1 and half -1 has mean 0, resid 0 and var 1: y = fl(fl(+-1 / sqrtf(fl(1 + eps))) * gamma) + beta in the fused
    kernel, and fl(+-inv * gamma) + beta with inv = fl(1 / sqrtf(fl(1 + eps))) in the general plan -- the same numbers, restated in numpy."""
    c, g, hw = HALF_CASES[case]
    e = (c // g) * int(np.prod(hw))
    assert e % 2 == 0
    sign = np.where(np.arange(e) < e // 2, 1.0, -1.0).astype(np.float32)
    x = np.broadcast_to(sign.reshape(1, 1, e), (3, g, e)).reshape((3, c) + tuple(hw))
    op = "InstanceNormalization" if g == c else "GroupNormalization"
    blob, spec = W.spatial_norm_model(c, g, hw, op=op, form="op21", **LAYOUTS[layout])
    gamma, beta = gamma_beta(spec)
    den = np.sqrt(np.float32(1.0) + np.float32(1e-5), dtype=np.float32)
    ga, be = per_element(gamma, c, hw), per_element(beta, c, hw)
    want = (x / den).astype(np.float32) * ga + be  # (each f32 operation rounded on its own; the general plan's +-inv is the same quotient)
    with serve(api, tmp_path, monkeypatch, blob, plan) as m:
        got = m(x)
    assert want.dtype == np.float32 and same_bits(got, want), float(np.abs(got.reshape(x.shape) - want).max())


# ---- bit identities ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan", list(PLANS))
def test_host_path_is_the_device_resident_slice(api, tmp_path, monkeypatch, plan):
    blob, spec = model_of("cg2_8x5x7", "cq_in_cq_out", "Silu")
    x = W.spatial_norm_inputs(spec, 70, seed=13).reshape(70, -1)
    with serve(api, tmp_path, monkeypatch, blob, plan) as m:
        host = m(x)
        dev = api.device_ordinal(0)
        d_in, d_out = api.DeviceBuffer(dev, x.nbytes).upload(x), api.DeviceBuffer(dev, host.nbytes)
        api.predict_device(m.name, d_in, 70, x.shape[1], d_out)
        assert same_bits(d_out.download(host.shape), host)
        api.predict_device(m.name, d_in, 3, x.shape[1], d_out, in_offset_bytes=20 * x.shape[1] * 4)
        assert same_bits(d_out.download((3, host.shape[1])), host[20:23])


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("back", ["const", "shape"])
def test_exporter_spelling_is_the_opset_21_operator(api, tmp_path, monkeypatch, back, layout):
    """inner scale 1 and inner B 0: the fold is exact, so both spellings carry the same gamma and beta and give the same bits"""
    outs = []
    for form in ("op21", "exporter"):
        blob, spec = W.spatial_norm_model(8, 2, (5, 7), op="GroupNormalization", form=form, back=back, act="Silu", **LAYOUTS[layout])
        with serve(api, tmp_path, monkeypatch, blob) as m:
            assert [k["kernel"] for k in m.plan["spatialnorm"]] == ["spatialnorm_fused"]
            outs.append(m(W.spatial_norm_inputs(spec, 5, seed=2)))
    assert same_bits(*outs)


@pytest.mark.parametrize("plan", list(PLANS))
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_a_nan_row_leaves_its_neighbours_alone(api, tmp_path, monkeypatch, layout, plan):
    blob, spec = model_of("cg2_8x5x7", layout, "Silu")
    x = W.spatial_norm_inputs(spec, 3, seed=5)
    bad = x.copy()
    bad[1, 3, 2, 4] = np.nan
    with serve(api, tmp_path, monkeypatch, blob, plan) as m:
        clean, dirty = m(x), m(bad)
    assert same_bits(dirty[0], clean[0]) and same_bits(dirty[2], clean[2])
    assert np.isnan(dirty[1]).any()


# ---- whole models ------------------------------------------------------------------------------------------------------------------
MODELS = {"style_net_small": lambda: W.style_net_small(), "unet_small_group": lambda: W.unet_small(norm="group")}


@pytest.mark.parametrize("model", list(MODELS))
def test_whole_models_at_the_parity_bar(api, tmp_path, monkeypatch, model):
    blob, spec = MODELS[model]()
    with serve(api, tmp_path, monkeypatch, blob) as m:
        assert m.plan["activation_layout"] == "NC/4HW4"
        assert m.plan["spatialnorm"] and all(k["kernel"] == "spatialnorm_fused" and k["in_layout"] == "NC/4HW4" and k["out_layout"] == "NC/4HW4" for k in m.plan["spatialnorm"])
        for n in (1, 3, 70):
            x = np.random.default_rng(30 + n).uniform(0, 1, size=(n,) + tuple(spec["in_shape"])).astype(np.float32)
            want = W.decoder_reference(spec, x).reshape(n, -1)
            ratio = bar_ratio(m(x), want)
            print(f"{model} rows={n}: max |err| / (rtol |ref| + atol) = {ratio:.4f}")
            assert ratio <= 1.0, (n, ratio)
