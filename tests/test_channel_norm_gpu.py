"""ConvNeXt's norm over the channel axis on the GPU, through predict_from_blob and predict_device.  Both
forms of the ChannelNorm kernel (channelnorm_regs, channelnorm_reread) on NCHW tensors and on channel-quad planes against the float64
reference at the parity bar of DESIGN.md section 5 (every element, at a common input offset of 0 and of 1000), the cases whose result is
known bit for bit, the bit identities (a row alone and in its batch, the call paths, unaligned results, two threads, the three spellings),
the ConvNeXt blocks whose channels-last spelling must give the bits of the same block spelled with Conv nodes, NaN / Inf pixels, and a small
whole ConvNeXt against a float64 torch twin.

Worst ratio to the bar, max |got - ref| / (1e-4 |ref| + 1e-6), measured on an MI355X (2026-10-18) over all parity cases: 0.3783 (C = 768,
NCHW, re-read form; channel quads 0.1816); register form 0.3002 (C = 512, NCHW; channel quads 0.1372); C <= 100 below 0.15 throughout.  torch's
float32 layer_norm over the permuted tensor on the CPU, same inputs and reference: 0.03 at offset 0 and 864 at offset 1000 (C = 3, 7 x 7:
three nearly equal values, whose variance is of the order of the first mean's rounding error -- what the second centring is for).  Blocks:
0.02-0.13, the same under INFERA_PRECISION=fp32.  The small ConvNeXt: kernel 0.0430, torch float32 0.0350."""
from __future__ import annotations

import threading

import numpy as np
import pytest

from infera_amd import onnx_writer as W
from tests import spatial_norm_cases as SC

try:
    import torch
except ImportError:  # the whole-model twin needs it
    torch = None

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 1e-6
REGS_MAX_C = 512         # host/channelnorm.hpp kChannelNormRegsMaxC
FORMS = {"regs": None, "reread": "0"}  # INFERA_CHANNELNORM_REGS
FRONTS = {"nchw": "relu", "quads": "conv"}
HWS = [(1, 1), (2, 3), (7, 7), (8, 8), (5, 13)]
# 1: a lone channel (d = 0); 3, 5: no quads; 4, 8, 12: quads in one wave; 96, 100: four waves, whole slices and a remainder; 512, 516:
# the largest C of the register form and the first beyond it; 768: the re-read form at ConvNeXt-T's last width
CHANNELS = [1, 3, 4, 5, 8, 12, 96, 100, REGS_MAX_C, REGS_MAX_C + 4, 768]
PARITY = [(c, layout, form) for c in CHANNELS for layout in FRONTS for form in FORMS
          if (layout == "nchw" or c % 4 == 0) and (form == "reread" or c <= REGS_MAX_C)]


@pytest.fixture(scope="module")
def api(built):
    from infera_amd import capi

    assert capi.device_count() >= 1, capi.get_devices()
    return capi


class Served:
    def __init__(self, api, tmp_path, blob, name="cn"):
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


def serve(api, tmp_path, monkeypatch, blob, form="regs", name="cn"):
    if FORMS[form] is None:
        monkeypatch.delenv("INFERA_CHANNELNORM_REGS", raising=False)
    else:
        monkeypatch.setenv("INFERA_CHANNELNORM_REGS", FORMS[form])  # (read when a model is loaded)
    return Served(api, tmp_path, blob, name)


def same_bits(got, want):
    got, want = np.ascontiguousarray(got, np.float32).reshape(-1), np.ascontiguousarray(want, np.float32).reshape(-1)
    return got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def bar_ratio(got, want):
    want = np.asarray(want, np.float64)
    return float((np.abs(np.asarray(got, np.float64).reshape(want.shape) - want) / (RTOL * np.abs(want) + ATOL)).max())


def check_step(m, c, layout, form):
    want_kernel = "channelnorm_regs" if form == "regs" and c <= REGS_MAX_C else "channelnorm_reread"
    want_layout = "NC/4HW4" if layout == "quads" and c % 4 == 0 else "NCHW"
    assert [(k["kernel"], k["in_layout"], k["out_layout"]) for k in m.plan["channelnorm"]] == [(want_kernel, want_layout, want_layout)], m.plan["channelnorm"]


# ---- the parity bar ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,layout,form", PARITY)
def test_parity_bar_at_offsets_0_and_1000(api, tmp_path, monkeypatch, c, layout, form):
    """max |got - ref| / (1e-4 |ref| + 1e-6) <= 1 against channelnorm_reference in float64 over every element, with x = offset + U(-1, 1),
    without an activation and with a fused Sigmoid, for 1, 3 and 70 rows of every extent: pixels per row that do not divide the tile of 64,
    tiles that span several images, the lone tail tile.  A row alone gives the bits it has inside its batch."""
    worst = 0.0
    for hw in HWS:
        for act in (None, "Sigmoid"):
            blob, spec = W.channel_norm_model(c, hw, spelling="layernorm2d", act=act, front=FRONTS[layout])
            with serve(api, tmp_path, monkeypatch, blob, form) as m:
                check_step(m, c, layout, form)
                assert norm_act(m) == act
                for offset in (0.0, 1000.0):
                    spec["offset"] = offset
                    for n in (1, 3, 70):
                        x = W.channel_norm_inputs(spec, n, seed=100 + n)
                        got = m(x)
                        ratio = bar_ratio(got, W.channel_norm_reference(spec, x).reshape(n, -1))
                        worst = max(worst, ratio)
                        assert ratio <= 1.0, (hw, act, offset, n, ratio)
                        if n > 1:
                            assert same_bits(m(x[n - 2:n - 1]), got[n - 2]), "a row alone differs from the row in its batch"
    print(f"\nC={c} {layout} {form}: worst max |err| / (rtol |ref| + atol) = {worst:.4f}")


def norm_act(m):
    (s,) = [s for s in m.plan["plan"]["steps"] if s["kind"] == "ChannelNorm"]
    return s.get("act")


@pytest.mark.parametrize("kind", list(SC.VALUE_KINDS))
def test_value_edges(api, tmp_path, monkeypatch, kind):
    """The same bar at the value edges of tests/spatial_norm_cases.py, one pixel's channels being one group: 2^40 U(-1, 1); 2^-20 U(-1, 1)
    under epsilon = 1e-12, comparable to the variance; 2^-10 U(-1, 1), where epsilon is 30 times the variance; one channel of every pixel
    at 1e4, also on a common offset of 1000.  (The Relu in front clips the negatives; the reference does the same.)"""
    hw, n, worst = (5, 13), 3, 0.0
    eps = SC.VALUE_KINDS[kind][1]
    for c, layout, form in [p for p in PARITY if p[0] in (3, 8, 100, REGS_MAX_C + 4)]:
        blob, spec = W.channel_norm_model(c, hw, spelling="layernorm2d", front=FRONTS[layout], eps=eps)
        with serve(api, tmp_path, monkeypatch, blob, form) as m:
            check_step(m, c, layout, form)
            for offset in (0.0, 1000.0) if kind == "outlier" else (0.0,):
                pixels = SC.value_groups(n * hw[0] * hw[1], c, kind, seed=400 + c, offset=offset)
                x = np.ascontiguousarray(pixels.reshape((n,) + hw + (c,)).transpose(0, 3, 1, 2))
                ratio = bar_ratio(m(x), W.channel_norm_reference(spec, x).reshape(n, -1))
                worst = max(worst, ratio)
                assert ratio <= 1.0, (c, layout, form, offset, ratio)
    print(f"\n{kind}: worst max |err| / (rtol |ref| + atol) = {worst:.4f}")


# ---- results known bit for bit -----------------------------------------------------------------------------------------------------
EXACT = [(c, layout, form) for c in (4, 6, 8, 96, 100, REGS_MAX_C, REGS_MAX_C + 4) for layout in FRONTS for form in FORMS
         if (layout == "nchw" or c % 4 == 0) and (form == "reread" or c <= REGS_MAX_C)]


@pytest.mark.parametrize("c,layout,form", EXACT)
def test_constant_pixels_give_the_activated_beta(api, tmp_path, monkeypatch, c, layout, form):
    """A pixel whose channels are all equal has d = 0 (the sums of C equal quarter-integers are exact), so y = act(beta[c]) exactly --
    also the pixel that holds 1000.25."""
    hw, n = (5, 13), 3
    vals = np.random.default_rng(3).integers(0, 65, size=(n, 1) + hw).astype(np.float32) / 4  # (>= 0: the Relu in front keeps them)
    vals[1, 0, 2, 7] = 1000.25
    x = np.broadcast_to(vals, (n, c) + hw)
    for act in (None, "Relu"):
        blob, spec = W.channel_norm_model(c, hw, spelling="nhwc_op", act=act, front=FRONTS[layout])
        beta = spec["beta"].reshape(1, c, 1, 1)
        want = np.broadcast_to(np.maximum(beta, 0) if act else beta, (n, c) + hw)
        with serve(api, tmp_path, monkeypatch, blob, form) as m:
            check_step(m, c, layout, form)
            got = m(x)
        assert same_bits(got, want), (act, float(np.abs(got.reshape(want.shape) - want).max()))


@pytest.mark.parametrize("c,layout,form", EXACT)
def test_half_plus_one_half_minus_one(api, tmp_path, monkeypatch, c, layout, form):
    """Half the channels at m + 1 and half at m - 1 with epsilon = 0: mean m, d = +-1, resid 0, var 1, and with gamma and beta small
    integers over 8 the pixel is +-gamma + beta exactly."""
    hw, n = (7, 7), 3
    mid = np.random.default_rng(4).integers(2, 40, size=(n, 1) + hw).astype(np.float32)  # (m - 1 >= 1 > 0: the Relu in front keeps them)
    sign = np.where(np.arange(c) % 2 == 0, 1.0, -1.0).astype(np.float32).reshape(1, c, 1, 1)
    x = mid + sign
    blob, spec = W.channel_norm_model(c, hw, spelling="channels_first", front=FRONTS[layout], eps=0.0, integer=True)
    want = sign * spec["gamma"].reshape(1, c, 1, 1) + spec["beta"].reshape(1, c, 1, 1)
    with serve(api, tmp_path, monkeypatch, blob, form) as m:
        check_step(m, c, layout, form)
        got = m(x)
    assert same_bits(got, np.broadcast_to(want, x.shape)), float(np.abs(got.reshape(x.shape) - want).max())


# ---- bit identities ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("c,layout", [(8, "nchw"), (8, "quads"), (100, "nchw"), (100, "quads")])
def test_call_paths_agree(api, tmp_path, monkeypatch, c, layout, form):
    """a row alone and inside a batch of 70, the host path and predict_device, a device-resident slice, two threads at once"""
    blob, spec = W.channel_norm_model(c, (5, 7), spelling="nhwc_op", act="Sigmoid", front=FRONTS[layout])
    x = W.channel_norm_inputs(spec, 70, seed=13)
    flat = np.ascontiguousarray(x.reshape(70, -1))
    with serve(api, tmp_path, monkeypatch, blob, form, name="paths") as m:
        ref = m(x)
        for i in (0, 33, 69):
            assert same_bits(m(x[i:i + 1]), ref[i]), i
        dev = api.device_ordinal(0)
        d_in, d_out = api.DeviceBuffer(dev, flat.nbytes).upload(flat), api.DeviceBuffer(dev, ref.nbytes)
        api.predict_device("paths", d_in, 70, flat.shape[1], d_out)
        assert same_bits(d_out.download(ref.shape), ref)
        api.predict_device("paths", d_in, 3, flat.shape[1], d_out, in_offset_bytes=20 * flat.shape[1] * 4)
        assert same_bits(d_out.download((3, ref.shape[1])), ref[20:23])
        outs, errs = [None, None], []

        def call(i):
            try:
                outs[i] = m(x[: 40 + 30 * i])
            except Exception as e:  # noqa: BLE001
                errs.append(e)

        ts = [threading.Thread(target=call, args=(i,)) for i in range(2)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not errs, errs
        assert same_bits(outs[0], ref[:40]) and same_bits(outs[1], ref[:70])


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("c,hw", [(8, (1, 1)), (8, (7, 7)), (96, (1, 1))])
def test_result_at_an_unaligned_address(api, tmp_path, monkeypatch, c, hw, form):
    """The step writes the served result itself (no convolution in the plan).  With H = W = 1 and whole quads the kernel reads and writes
    quads, by 16-byte accesses only where both pointers allow: a result 4 or 8 bytes past a 16-byte boundary takes element accesses, with the
    same bits."""
    blob, spec = W.channel_norm_model(c, hw, spelling="nhwc_op", front="relu")
    x = W.channel_norm_inputs(spec, 5, seed=4)
    flat = np.ascontiguousarray(x.reshape(5, -1))
    with serve(api, tmp_path, monkeypatch, blob, form, name="unaligned") as m:
        want = m(x)
        assert bar_ratio(want, W.channel_norm_reference(spec, x).reshape(5, -1)) <= 1.0
        dev = api.device_ordinal(0)
        d_in, d_out = api.DeviceBuffer(dev, flat.nbytes).upload(flat), api.DeviceBuffer(dev, want.nbytes + 16)
        for off in (0, 4, 8):
            api.predict_device("unaligned", d_in, 5, flat.shape[1], d_out, out_offset_bytes=off)
            got = d_out.download((want.size + 4,))[off // 4: off // 4 + want.size]
            assert same_bits(got, want), off


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("layout", list(FRONTS))
def test_three_spellings_give_the_same_bits(api, tmp_path, monkeypatch, layout, form):
    outs = []
    for sp in ("nhwc_op", "layernorm2d", "channels_first"):
        blob, spec = W.channel_norm_model(12, (5, 7), spelling=sp, act="Relu", post_affine=True, front=FRONTS[layout])
        with serve(api, tmp_path, monkeypatch, blob, form) as m:
            outs.append(m(W.channel_norm_inputs(spec, 5, seed=2)))
    assert same_bits(outs[0], outs[1]) and same_bits(outs[0], outs[2])
    assert bar_ratio(outs[0], W.channel_norm_reference(spec, W.channel_norm_inputs(spec, 5, seed=2)).reshape(5, -1)) <= 1.0


# ---- blocks ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["default", "fp32"])
@pytest.mark.parametrize("hw", [(7, 7), (8, 8)])
@pytest.mark.parametrize("c", [8, 96])
def test_blocks_give_the_bits_of_the_nchw_block(api, tmp_path, monkeypatch, c, hw, precision):
    """The torchvision and Hugging Face blocks give the bits of the same block spelled with the channels-first norm and Conv 1x1 nodes: the
    channels-last detour costs nothing and changes nothing.  Layer scale folds into the second 1x1 convolution's weights and bias in all
    three spellings -- behind the bias Add in each --, so no case needs the weaker comparison against float64; the bar is asserted as well."""
    if precision == "fp32":
        monkeypatch.setenv("INFERA_PRECISION", "fp32")
    else:
        monkeypatch.delenv("INFERA_PRECISION", raising=False)
    outs = {}
    for gelu in ("op", "decomposed"):
        for style in ("nchw", "torchvision", "hf"):
            blob, spec = W.convnext_block_model(c, hw, style=style, gelu=gelu, weight_scale=0.5)
            x = np.random.default_rng(21).uniform(-1, 1, (5, c) + hw).astype(np.float32)
            with serve(api, tmp_path, monkeypatch, blob) as m:
                assert m.plan["activation_layout"] == "NC/4HW4"
                outs[style] = m(x)
        assert same_bits(outs["torchvision"], outs["nchw"]), gelu
        assert same_bits(outs["hf"], outs["nchw"]), gelu
        ratio = bar_ratio(outs["nchw"], W.convnext_block_reference(spec, x).reshape(5, -1))
        print(f"\nblock C={c} {hw} {precision} gelu={gelu}: max |err| / (rtol |ref| + atol) = {ratio:.4f}")
        assert ratio <= 1.0, ratio


# ---- NaN / Inf ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("c", [6, 8, 100])
def test_nan_and_inf_stay_in_their_pixels(api, tmp_path, monkeypatch, c, form):
    """A NaN and an Inf in two pixels of image 2 leave every other image and every other pixel of image 2 with their bits (the identity
    1x1 layers around the norm mix the channels of a pixel, never pixels); the two pixels are not finite."""
    hw = (5, 7)
    blob, spec = W.channel_norm_model(c, hw, spelling="layernorm2d", front="conv")
    x = W.channel_norm_inputs(spec, 4, seed=5)
    bad = x.copy()
    bad[2, 1, 0, 3] = np.nan
    bad[2, c - 1, 4, 6] = np.inf
    with serve(api, tmp_path, monkeypatch, blob, form) as m:
        clean, dirty = m(x).reshape(x.shape), m(bad).reshape(x.shape)
    hit = np.zeros(x.shape, bool)
    hit[2, :, 0, 3] = hit[2, :, 4, 6] = True
    assert same_bits(dirty[~hit], clean[~hit])
    assert not np.isfinite(dirty[hit]).any()


# ---- the whole model ---------------------------------------------------------------------------------------------------------------
def make_twin(img, widths, depths, classes, seed, w_scale):
    nn = torch.nn

    class Block(nn.Module):
        def __init__(self, c):
            super().__init__()
            self.dw, self.norm = nn.Conv2d(c, c, 7, padding=3, groups=c), nn.LayerNorm(c, eps=1e-6)
            self.fc1, self.fc2 = nn.Linear(c, 4 * c), nn.Linear(4 * c, c)
            self.ls = nn.Parameter(torch.rand(c) * 0.75 + 0.25)

        def forward(self, x):
            h = torch.nn.functional.layer_norm(self.dw(x).permute(0, 2, 3, 1), self.norm.normalized_shape, self.norm.weight, self.norm.bias, 1e-6)
            h = self.fc2(torch.nn.functional.gelu(self.fc1(h)))
            return x + (self.ls.view(-1, 1, 1) * h.permute(0, 3, 1, 2))

    class Norm2d(nn.LayerNorm):
        def forward(self, x):
            return torch.nn.functional.layer_norm(x.permute(0, 2, 3, 1), self.normalized_shape, self.weight, self.bias, self.eps).permute(0, 3, 1, 2)

    class Twin(nn.Module):
        def __init__(self):
            super().__init__()
            torch.manual_seed(seed)
            self.stem, self.stem_norm = nn.Conv2d(img[0], widths[0], 4, 4), Norm2d(widths[0], eps=1e-6)
            self.down = nn.ModuleList([nn.ModuleList([Norm2d(widths[i - 1], eps=1e-6), nn.Conv2d(widths[i - 1], widths[i], 2, 2)]) for i in range(1, len(widths))])
            self.stages = nn.ModuleList([nn.ModuleList([Block(c) for _ in range(d)]) for c, d in zip(widths, depths)])
            self.head_norm, self.head = Norm2d(widths[-1], eps=1e-6), nn.Linear(widths[-1], classes)
            with torch.no_grad():
                for name, prm in self.named_parameters():
                    if "norm" in name:  # gamma in [0.5, 1.5], beta in [-0.5, 0.5]
                        prm.copy_(torch.rand_like(prm) + (0.5 if name.endswith("weight") else -0.5))
                    elif not name.endswith("ls"):
                        prm.mul_(w_scale)
            self.eval()

        def forward(self, x):
            h = self.stem_norm(self.stem(x))
            for i, blocks in enumerate(self.stages):
                if i > 0:
                    h = self.down[i - 1][1](self.down[i - 1][0](h))
                for b in blocks:
                    h = b(h)
            return self.head(self.head_norm(h.mean((2, 3), keepdim=True)).flatten(1))

        def spec(self):
            f = lambda p: p.detach().cpu().numpy().astype(np.float32)  # noqa: E731
            blk = lambda b: {"dw_W": f(b.dw.weight), "dw_b": f(b.dw.bias), "g": f(b.norm.weight), "b": f(b.norm.bias), "W1": f(b.fc1.weight).T.copy(),  # noqa: E731
                             "b1": f(b.fc1.bias), "W2": f(b.fc2.weight).T.copy(), "b2": f(b.fc2.bias), "ls": f(b.ls)}
            return {"img": tuple(img), "widths": tuple(widths), "depths": tuple(depths), "classes": classes, "eps": float(np.float32(1e-6)),
                    "stem_W": f(self.stem.weight), "stem_b": f(self.stem.bias), "stem_norm": (f(self.stem_norm.weight), f(self.stem_norm.bias)),
                    "down": [{"norm": (f(d[0].weight), f(d[0].bias)), "W": f(d[1].weight), "b": f(d[1].bias)} for d in self.down],
                    "stages": [[blk(b) for b in blocks] for blocks in self.stages],
                    "head_norm": (f(self.head_norm.weight), f(self.head_norm.bias)), "head_W": f(self.head.weight).T.copy(), "head_b": f(self.head.bias)}

    return Twin()


def run_twin(twin, x, dtype):
    import copy

    with torch.no_grad():
        return copy.deepcopy(twin).to(dtype)(torch.from_numpy(x).to(dtype)).double().numpy()


W_SCALE = 0.5  # torch float32 on the CPU then stays within a quarter of the bar against float64 (asserted below)


@pytest.mark.parametrize("style", ["torchvision", "hf"])
def test_small_convnext_against_torch_float64(api, tmp_path, monkeypatch, style):
    if torch is None:
        pytest.skip("torch is not installed")
    monkeypatch.delenv("INFERA_CHANNELNORM_REGS", raising=False)
    twin = make_twin((3, 32, 32), (8, 16), (1, 1), 5, seed=17, w_scale=W_SCALE)
    x = np.random.default_rng(5).uniform(-1, 1, (37, 3, 32, 32)).astype(np.float32)
    ref, ref32 = run_twin(twin, x, torch.float64), run_twin(twin, x, torch.float32)
    r32 = bar_ratio(ref32, ref)
    spec = twin.spec()
    with Served(api, tmp_path, W.convnext_from_spec(spec, style=style)) as m:
        assert [s["kind"] for s in m.plan["plan"]["steps"]].count("ChannelNorm") == 5 and m.plan["activation_layout"] == "NC/4HW4"
        rk = bar_ratio(m(x), ref)
    print(f"\nconvnext {style}: torch-f32 {r32:.4f} kernel {rk:.4f}")
    assert r32 <= 0.25, r32
    assert rk <= 1.0, rk
    # the writer's own float64 restatement agrees with the twin far inside the bar
    assert bar_ratio(W.convnext_reference(spec, x), ref) < 1e-3
