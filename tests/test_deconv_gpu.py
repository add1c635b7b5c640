"""ConvTranspose, Resize and Upsample on the GPU.  Transposed convolutions on whole-number data against the float64
reference BIT FOR BIT -- on the MFMA phase kernel and on the generic kernel, writing channel-quad planes and NCHW --, on generic data within
the derived bound of a k-ordered fp32 chain, the bit identities (a row alone and in its batch, the two output layouts, the host path and
the device-resident entry), the empty phase of a kernel shorter than its stride, Resize in every mode, and the writer's decoder models
against their float64 evaluation at the project's parity bar."""
from __future__ import annotations

import numpy as np
import pytest

from infera_amd import onnx_writer as W

from deconv_cases import GEOMETRIES, geometry, small_ints

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 1e-6
ROWS = (1, 3, 70)
# how the layer under test is embedded: identity 1x1 layers around it put it on channel-quad tensors (the model's own input and a served
# [C,H,W] result are NCHW)
LAYOUTS = {"cq_in_cq_out": dict(pre=True, post=True), "cq_in_nchw_out": dict(pre=True, post=False), "nchw_in_nchw_out": dict(pre=False, post=False)}
KERNELS = {"mfma": None, "generic": "0"}


@pytest.fixture(scope="module")
def api(built):
    from infera_amd import capi

    assert capi.device_count() >= 1, capi.get_devices()
    return capi


class Served:
    def __init__(self, api, tmp_path, blob, name="dc"):
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


def serve(api, tmp_path, monkeypatch, blob, kernel="mfma", name="dc"):
    if KERNELS[kernel] is None:
        monkeypatch.delenv("INFERA_CONVT_MFMA", raising=False)
    else:
        monkeypatch.setenv("INFERA_CONVT_MFMA", KERNELS[kernel])  # (read when a model is loaded)
    return Served(api, tmp_path, blob, name)


def same_bits(got, want):
    got, want = np.ascontiguousarray(got, np.float32).reshape(-1), np.ascontiguousarray(want, np.float32).reshape(-1)
    return got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def expected_kernel(g, layout, kernel):
    mfma = kernel == "mfma" and LAYOUTS[layout]["pre"] and g.get("g", 1) == 1 and g["C"] % 4 == 0 and (g["M"] % 4 == 0 or not LAYOUTS[layout]["post"])
    return "convt2d_phase" if mfma else "convt2d_generic"


def layer_of(spec, name="convt"):
    return next(p for op, out, ins, p in spec["layers"] if out == name)


def check_exact(api, tmp_path, monkeypatch, g, layout, kernel, act=None, rows=ROWS):
    blob, spec = W.conv_transpose_model(g, integer=True, act=act, **LAYOUTS[layout])
    with serve(api, tmp_path, monkeypatch, blob, kernel) as m:
        assert m.plan["convt"][0]["kernel"] == expected_kernel(g, layout, kernel), m.plan["convt"]
        if LAYOUTS[layout]["pre"] and g["C"] % 4 == 0 and g["M"] % 4 == 0:
            assert m.plan["convt"][0]["in_layout"] == "NC/4HW4"
            assert m.plan["convt"][0]["out_layout"] == ("NC/4HW4" if LAYOUTS[layout]["post"] else "NCHW")
        for n in rows:
            x = small_ints(100 + n, (n,) + tuple(spec["in_shape"]))
            want = W.decoder_reference(spec, x).astype(np.float32)
            got = m(x)
            assert same_bits(got, want), (n, float(np.abs(got.reshape(want.shape) - want).max()))


# ---- exact cases: every partial sum is a whole number below 2^24, so any order of summation gives the one right answer ----------------
# (the model's own NCHW input is read by the generic kernel under either setting: one case)
LAYOUT_KERNEL = [(l, k) for l in LAYOUTS for k in KERNELS if not (l == "nchw_in_nchw_out" and k == "mfma")]


@pytest.mark.parametrize("layout,kernel", LAYOUT_KERNEL)
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_exact_c32_m32_5x5(api, tmp_path, monkeypatch, name, layout, kernel):
    """C = M = 32 on 5 x 5: a phase has 25 pixels or fewer (one partial tile); 1, 3 and 70 rows: tiles and workgroups cross images."""
    check_exact(api, tmp_path, monkeypatch, geometry(name, 32, 32, 5, 5), layout, kernel)


_BOTH = ("cq_in_cq_out", "cq_in_nchw_out")
# channel and feature tails; three output channels (NCHW out only); three input channels (no quads: generic only); 1-D.  (C, M, H, layouts, kernels)
SHAPES = {"tails_40_36": (40, 36, 5, _BOTH, tuple(KERNELS)), "m3_nchw_out": (64, 3, 5, ("cq_in_nchw_out",), tuple(KERNELS)),
          "c3": (3, 8, 5, ("nchw_in_nchw_out",), ("generic",)), "conv1d_L7": (32, 32, None, _BOTH, tuple(KERNELS))}


def admits(shape, name):
    """four groups need channel and feature counts that are multiples of four (depthwise takes M = C)"""
    C, M = SHAPES[shape][:2]
    return GEOMETRIES[name].get("g") != 4 or (C % 4 == 0 and M % 4 == 0)


SHAPE_CASES = [pytest.param(shape, name, k, id=f"{shape}-{name}-{k}") for shape in SHAPES for name in GEOMETRIES if admits(shape, name) for k in SHAPES[shape][4]]


@pytest.mark.parametrize("shape,name,kernel", SHAPE_CASES)
def test_exact_tails_and_1d(api, tmp_path, monkeypatch, shape, name, kernel):
    C, M, H, layouts, _ = SHAPES[shape]
    for layout in layouts:
        check_exact(api, tmp_path, monkeypatch, geometry(name, C, M, H, 7 if H is None else 5), layout, kernel, act="Relu", rows=(3, 70))


def test_empty_phase_stores_the_activated_bias(api, tmp_path, monkeypatch):
    g = geometry("k1_s2", 32, 32, 5, 5)
    for kernel in KERNELS:
        for layout in ("cq_in_cq_out", "cq_in_nchw_out"):
            blob, spec = W.conv_transpose_model(g, integer=True, act="Relu", **LAYOUTS[layout])
            b = layer_of(spec)["b"]
            assert (b > 0).any() and (b < 0).any()
            with serve(api, tmp_path, monkeypatch, blob, kernel) as m:
                got = m(small_ints(7, (3, 32, 5, 5))).reshape(3, 32, 9, 9)
            relu_b = np.maximum(b, 0.0)[None, :, None, None]
            assert np.array_equal(got[:, :, 1::2, :], np.broadcast_to(relu_b, (3, 32, 4, 9)))
            assert np.array_equal(got[:, :, :, 1::2], np.broadcast_to(relu_b, (3, 32, 9, 4)))


# ---- generic data ------------------------------------------------------------------------------------------------------------------
def chain_bound(spec, x):
    """(K + 2) 2^-24 (sum |x| |w| + |b|) per element, K = (C / g) kh kw terms: the bound tests/dense_ref.py derives for a k-ordered chain of
    fp32 multiply-adds (zero padding and skipped taps add no rounding)."""
    p = layer_of(spec)
    if x.ndim == 3:  # (the 1-D form keeps its weights as [C, M/g, 1, k])
        return chain_bound(spec, x[:, :, None, :])[:, :, 0, :]
    mag = W.conv_transpose_reference(np.abs(x), np.abs(p["w"]), np.abs(p["b"]), p["strides"], p["pads"], p["dilations"], p["groups"], p["output_padding"])
    K = (p["w"].shape[0] // p["groups"]) * p["w"].shape[2] * p["w"].shape[3]
    return (K + 2) * 2.0 ** -24 * mag


def check_generic(api, tmp_path, monkeypatch, g, layouts, kernel, label):
    outs = {}
    for layout in layouts:
        blob, spec = W.conv_transpose_model(g, **LAYOUTS[layout])
        x = np.random.default_rng(11).normal(size=(70,) + tuple(spec["in_shape"])).astype(np.float32)
        want, bound = W.decoder_reference(spec, x), chain_bound(spec, x.astype(np.float64))
        with serve(api, tmp_path, monkeypatch, blob, kernel) as m:
            assert m.plan["convt"][0]["kernel"] == expected_kernel(g, layout, kernel)
            got = m(x).reshape(want.shape)
            alone = m(x[41:42])
        excess = np.abs(got - want) - bound
        print(f"{label} {kernel} {layout}: max |err| / bound = {float((np.abs(got - want) / np.maximum(bound, 1e-300)).max()):.3f}")
        assert float(excess.max()) <= 0.0, (layout, float(excess.max()))
        assert same_bits(alone, got[41]), "a row alone differs from the row in its batch of 70"
        outs[layout] = got
    if len(outs) == 2:
        assert same_bits(*outs.values()), "the channel-quad and the NCHW output differ"


@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_generic_data_within_the_chain_bound(api, tmp_path, monkeypatch, name, kernel):
    check_generic(api, tmp_path, monkeypatch, geometry(name, 32, 32, 5, 5), _BOTH, kernel, f"{name} C=32 M=32")


@pytest.mark.parametrize("shape,name,kernel", SHAPE_CASES)
def test_generic_data_tails_and_1d(api, tmp_path, monkeypatch, shape, name, kernel):
    """The chain bound, the row-alone identity and (where both exist) the identity of the two output layouts on the shapes of the exact list:
    the M-padded three-channel NCHW-out layer, three input channels, channel and feature tails, the 1-D form."""
    C, M, H, layouts, _ = SHAPES[shape]
    check_generic(api, tmp_path, monkeypatch, geometry(name, C, M, H, 7 if H is None else 5), layouts, kernel, f"{shape} {name}")


def test_host_path_is_the_device_resident_slice(api, tmp_path, monkeypatch):
    blob, spec = W.conv_transpose_model(geometry("k4_s2_p1", 32, 32, 5, 5), act="Relu", **LAYOUTS["cq_in_nchw_out"])
    x = np.random.default_rng(13).normal(size=(70, 32 * 5 * 5)).astype(np.float32)
    for kernel in KERNELS:
        with serve(api, tmp_path, monkeypatch, blob, kernel) as m:
            host = m(x)
            dev = api.device_ordinal(0)
            d_in, d_out = api.DeviceBuffer(dev, x.nbytes).upload(x), api.DeviceBuffer(dev, host.nbytes)
            api.predict_device(m.name, d_in, 70, x.shape[1], d_out)
            assert same_bits(d_out.download(host.shape), host)
            api.predict_device(m.name, d_in, 3, x.shape[1], d_out, in_offset_bytes=20 * x.shape[1] * 4)
            assert same_bits(d_out.download((3, host.shape[1])), host[20:23])


# ---- Resize ------------------------------------------------------------------------------------------------------------------------
def resize_cases(c):
    """(pre, post) embeddings: NCHW always, channel-quad planes where the channels are whole quads"""
    return [dict(pre=False, post=False)] + ([dict(pre=True, post=True)] if c % 4 == 0 else [])


@pytest.mark.parametrize("c", [3, 8])
@pytest.mark.parametrize("coord", ["half_pixel", "pytorch_half_pixel", "asymmetric", "align_corners"])
@pytest.mark.parametrize("nearest_mode", ["round_prefer_floor", "round_prefer_ceil", "floor", "ceil"])
def test_resize_nearest_bit_for_bit(api, tmp_path, monkeypatch, nearest_mode, coord, c):
    for embed in resize_cases(c):
        for kw in (dict(scales=(2.0, 3.0)), dict(sizes=(8, 7))):
            blob, spec = W.resize_model(c, (5, 4), mode="nearest", coord=coord, nearest_mode=nearest_mode, **kw, **embed)
            with serve(api, tmp_path, monkeypatch, blob) as m:
                for n in (1, 5):
                    x = np.random.default_rng(n).normal(size=(n, c, 5, 4)).astype(np.float32)
                    assert same_bits(m(x), W.decoder_reference(spec, x).astype(np.float32))


@pytest.mark.parametrize("c", [3, 8])
@pytest.mark.parametrize("coord,hw,kw", [("half_pixel", (5, 6), dict(scales=(2.0, 2.0))), ("asymmetric", (5, 6), dict(scales=(2.0, 2.0))),
                                         ("pytorch_half_pixel", (5, 6), dict(scales=(2.0, 2.0))), ("align_corners", (4, 4), dict(sizes=(7, 7)))])
def test_resize_linear_dyadic_weights_bit_for_bit(api, tmp_path, monkeypatch, coord, hw, kw, c):
    """x2 and align_corners 4 -> 7: every weight is a multiple of 1/4 and the data whole numbers up to 8, so every product and sum is exact."""
    for embed in resize_cases(c):
        blob, spec = W.resize_model(c, hw, mode="linear", coord=coord, **kw, **embed)
        with serve(api, tmp_path, monkeypatch, blob) as m:
            for n in (1, 5):
                x = small_ints(n, (n, c) + hw)
                assert same_bits(m(x), W.decoder_reference(spec, x).astype(np.float32))


@pytest.mark.parametrize("c", [3, 8])
@pytest.mark.parametrize("coord", ["half_pixel", "align_corners", "asymmetric"])
def test_resize_linear_5_to_8_within_bound(api, tmp_path, monkeypatch, coord, c):
    """Every element within 8 * 2^-24 * max |x| over its four taps of the float64 reference (weights in float64, as the specification
    defines them): six roundings of a convex combination -- per axis the weight pair, the product and the fused multiply-add --, two units
    for second-order terms.  (align_corners 5 -> 8 has the weights frac(4 o / 7): not dyadic.)"""
    for embed in resize_cases(c):
        blob, spec = W.resize_model(c, (5, 5), sizes=(8, 8), mode="linear", coord=coord, **embed)
        with serve(api, tmp_path, monkeypatch, blob) as m:
            for n in (1, 5):
                x = np.random.default_rng(20 + n).normal(size=(n, c, 5, 5)).astype(np.float32)
                want = W.decoder_reference(spec, x)
                y0, y1, _ = W.resize_axis_reference(5, 8, 8 / 5, "linear", coord)
                ax = np.abs(x.astype(np.float64))
                taps = np.maximum(np.maximum(ax[:, :, y0][:, :, :, y0], ax[:, :, y0][:, :, :, y1]), np.maximum(ax[:, :, y1][:, :, :, y0], ax[:, :, y1][:, :, :, y1]))
                err = np.abs(m(x).reshape(want.shape) - want)
                print(f"linear 5->8 {coord} C={c} {embed}: max err / bound = {float((err / (8 * 2.0 ** -24 * taps)).max()):.3f}")
                assert float((err - 8 * 2.0 ** -24 * taps).max()) <= 0.0


def test_resize_1d_and_upsample(api, tmp_path, monkeypatch):
    for blob, spec in (W.resize_model(8, (7,), scales=(2.0,), mode="linear", coord="half_pixel"), W.resize_model(8, (7,), sizes=(10,), mode="nearest", coord="asymmetric", nearest_mode="floor"),
                       W.resize_model(4, (5, 4), scales=(2.0, 2.0), mode="nearest", op="Upsample", opset=9), W.resize_model(4, (5, 4), scales=(2.0, 2.0), mode="linear", op="Upsample", opset=7)):
        with serve(api, tmp_path, monkeypatch, blob) as m:
            x = small_ints(3, (5,) + tuple(spec["in_shape"]))
            assert same_bits(m(x), W.decoder_reference(spec, x).astype(np.float32))


# ---- whole models ------------------------------------------------------------------------------------------------------------------
MODELS = {"conv_autoencoder": lambda: W.conv_autoencoder((3, 16, 32), 16), "unet_small": lambda: W.unet_small(3, 3, 16),
          "upsample_decoder": lambda: W.upsample_decoder((8, 4, 4), 3), "conv1d_autoencoder": lambda: W.conv1d_autoencoder(16, 4)}


@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("model", list(MODELS))
def test_whole_models_at_the_parity_bar(api, tmp_path, monkeypatch, model, kernel):
    blob, spec = MODELS[model]()
    with serve(api, tmp_path, monkeypatch, blob, kernel) as m:
        for n in (1, 9):
            x = np.random.default_rng(30 + n).uniform(0, 1, size=(n,) + tuple(spec["in_shape"])).astype(np.float32)
            want = W.decoder_reference(spec, x).reshape(n, -1)
            got = m(x)
            excess = np.abs(got - want) - (RTOL * np.abs(want) + ATOL)
            print(f"{model} {kernel} rows={n}: max rel err {float((np.abs(got - want) / np.maximum(np.abs(want), 1e-6)).max()):.3e}")
            assert float(excess.max()) <= 0.0, (n, float(excess.max()))
            if model == "conv1d_autoencoder":  # a flat table through infera_predict
                assert same_bits(api.predict(m.name, x), got)
