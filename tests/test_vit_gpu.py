"""The Tokens step and ViT-shaped models on the GPU: the step alone bit for bit against numpy (a copy plus one IEEE addition), whole models
against a float64 torch twin at the project's bar, and the call paths against each other.

Worst ratios to the bar measured on an MI355X (kernel / torch float32 on the CPU): see the commit that added this file."""
import threading

import numpy as np
import pytest

from infera_amd import onnx_writer as W

try:  # (only the whole-model tests need torch: the step's own tests run without it)
    import torch
except ImportError:
    torch = None
pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 1e-6  # the bar of tests/test_transformer_gpu.py


@pytest.fixture(scope="module")
def api(built):
    from infera_amd import capi

    assert capi.device_count() >= 1, capi.get_devices()
    return capi


def worst_ratio(got, ref):
    """max over the elements of |got - ref| / (RTOL |ref| + ATOL): <= 1 passes the bar."""
    got, ref = np.asarray(got, np.float64).reshape(-1), np.asarray(ref, np.float64).reshape(-1)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.max(np.abs(got - ref) / (RTOL * np.abs(ref) + ATOL)))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32).reshape(-1), np.ascontiguousarray(b, np.float32).reshape(-1)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


class Served:
    def __init__(self, api, tmp_path, blob, name="vit"):
        self.api, self.name = api, name
        api.load_model(name, W.write(str(tmp_path / f"{name}.onnx"), blob))

    def __call__(self, x):
        """the host path for [N, C, H, W] inputs: predict_from_blob (infera_predict takes rank-2 tables only)"""
        x = np.ascontiguousarray(x, np.float32)
        return self.api.predict_from_blob(self.name, x.tobytes()).reshape(len(x), -1)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.api.unload_model(self.name)


def images(rows, c, hw, seed=0):
    """small integers over 8 with both signs: every product and sum the exact fronts make of them is exact"""
    return (np.random.default_rng(seed).integers(-256, 256, (rows, c) + tuple(hw)) / 8.0).astype(np.float32)


# ---- the step alone, bit for bit ---------------------------------------------------------------------------------------------------------
CS = [1, 3, 4, 5, 8, 64, 68]
HWS = [(1, 1), (2, 3), (7, 9), (8, 8), (5, 13), (14, 14)]


@pytest.mark.parametrize("c", CS)
def test_step_from_nchw_is_exact(api, tmp_path, c):
    """front = Relu on the model input: the NCHW kernel, both access widths on both sides, partial tiles, tiles of many images"""
    for hw in HWS:
        for prefix in (0, 1, 2):
            blob, spec = W.tokens_model(c, hw, prefix=prefix, pos=prefix != 1 or hw == (7, 9), front="relu", view=("flatten", "reshape", "shape_subgraph")[prefix])
            with Served(api, tmp_path, blob) as m:
                plan = m.api.get_plan(m.name)
                if prefix == 0 and (c == 1 or hw == (1, 1)):  # (nothing moves and nothing is joined: the alias it always was)
                    assert "tokens" not in plan
                else:
                    assert plan["tokens"][0]["in_layout"] == "NCHW"
                for rows in (1, 3, 70):
                    x = images(rows, c, hw, seed=rows)
                    want = W.tokens_reference(spec, x)
                    got = m(x)
                    assert same_bits(got, want), (c, hw, prefix, rows)


@pytest.mark.parametrize("c", [4, 8, 64, 68, 6, 5])
def test_step_behind_a_convolution_is_exact(api, tmp_path, c):
    """front = a 1x1 convolution by twice the identity: channel-quad planes where c % 4 == 0, the NCHW kernel behind a generic convolution else"""
    for hw in ((2, 3), (7, 9), (8, 8), (14, 14)):
        for prefix in (0, 2):
            blob, spec = W.tokens_model(c, hw, prefix=prefix, pos=True, front="conv")
            with Served(api, tmp_path, blob) as m:
                assert m.api.get_plan(m.name)["tokens"][0]["in_layout"] == ("NC/4HW4" if c % 4 == 0 else "NCHW")
                for rows in (1, 3, 70):
                    x = images(rows, c, hw, seed=rows)
                    assert same_bits(m(x), W.tokens_reference(spec, x)), (c, hw, prefix, rows)


@pytest.mark.parametrize("front", ["relu", "conv"])
def test_result_at_an_unaligned_address(api, tmp_path, front):
    """C % 4 == 0 and S % 4 == 0, so only the pointer decides: a device-resident result 4 bytes past a 16-byte boundary takes the word
    stores (hip/tokens.hip: y_ok), with the bits of the 16-byte ones.  (The step's input is always a buffer of the plan's own.)"""
    c, hw = 8, (8, 8)
    blob, spec = W.tokens_model(c, hw, prefix=1, pos=True, front=front)
    x = images(5, c, hw, seed=4)
    want = W.tokens_reference(spec, x).reshape(5, -1)
    flat = np.ascontiguousarray(x.reshape(5, -1))
    with Served(api, tmp_path, blob, name="unaligned") as m:
        dev = api.device_ordinal(0)
        d_in, d_out = api.DeviceBuffer(dev, flat.nbytes), api.DeviceBuffer(dev, want.nbytes + 16)
        d_in.upload(flat)
        for off in (0, 4, 8):
            api.predict_device("unaligned", d_in, 5, flat.shape[1], d_out, out_offset_bytes=off)
            got = d_out.download((want.size + 4,))[off // 4: off // 4 + want.size]
            assert same_bits(got, want), off


@pytest.mark.parametrize("front", ["relu", "conv"])
def test_vit_base_width(api, tmp_path, front):
    blob, spec = W.tokens_model(768, (14, 14), prefix=1, pos=True, front=front)
    x = images(3, 768, (14, 14), seed=9)
    with Served(api, tmp_path, blob) as m:
        assert same_bits(m(x), W.tokens_reference(spec, x))


@pytest.mark.parametrize("front", ["neg", "conv"])
def test_nan_and_inf_stay_in_their_image(api, tmp_path, front):
    """A NaN and an Inf in image 2.  The other images keep their bits.  front = Neg hands both to the NCHW kernel as they are (Relu would
    turn the NaN into 0), so image 2 is the reference with one NaN and one Inf; behind the 1x1 convolution (channel quads) 0 * NaN and
    0 * Inf spread over the channels of the two poisoned pixels, so there image 2 keeps the bits of every other window row."""
    P, hw = 1, (7, 9)
    blob, spec = W.tokens_model(8, hw, prefix=P, pos=True, front=front)
    x = images(5, 8, hw, seed=2)
    with Served(api, tmp_path, blob) as m:
        clean = m(x)
        assert same_bits(clean, W.tokens_reference(spec, x))
        bad = x.copy()
        bad[2, 3, 4, 5], bad[2, 0, 0, 0] = np.nan, np.inf
        got = m(bad)
    assert same_bits(np.delete(got, 2, axis=0), np.delete(clean, 2, axis=0))
    got2, clean2 = got[2].reshape(P + 63, 8), clean[2].reshape(P + 63, 8)
    hit = [P + 4 * 9 + 5, P + 0]  # the window rows of the two pixels
    assert same_bits(np.delete(got2, hit, axis=0), np.delete(clean2, hit, axis=0))
    assert not np.isfinite(got2[hit[0]]).all() and not np.isfinite(got2[hit[1]]).all()
    if front == "neg":
        assert np.array_equal(got2, W.tokens_reference(spec, bad)[2], equal_nan=True)
        assert np.isnan(got2).sum() == 1 and np.isinf(got2).sum() == 1 and np.isnan(got2[hit[0], 3]) and got2[hit[1], 0] == -np.inf


def test_fused_and_unfused_position_add_give_the_same_bits(api, tmp_path):
    """x + pos in the step's store, and as the BinaryConst a second reader leaves: random f32 tables, so that the sums round.  The table is
    >= 0, so the second reader's Max(tokens + pos, tokens) is tokens + pos itself (rounding is monotone) and the outputs compare whole."""
    rng = np.random.default_rng(3)
    c, hw, P = 8, (7, 9), 1
    cls, pos = rng.standard_normal((P, c)).astype(np.float32), np.abs(rng.standard_normal((P + 63, c))).astype(np.float32)
    x = rng.standard_normal((70, c) + hw).astype(np.float32)
    outs = []
    for second in (False, True):
        nodes, inits = [W.node("Relu", ["X"], ["front"])], []
        out = W.token_nodes(nodes, inits, "front", c, hw, [cls], pos, second_reader=second)
        blob = W.model("pos", nodes, inits, [W.value_info("X", ["N", c] + list(hw))], [W.value_info(out, ["N", P + 63, c])], opset=13)
        with Served(api, tmp_path, blob) as m:
            kinds = [s["kind"] for s in m.api.get_plan(m.name)["plan"]["steps"]]
            assert ("BinaryConst" in kinds) == second, kinds
            outs.append(m(x))
    tok = np.concatenate([np.broadcast_to(cls[None], (70, P, c)), np.maximum(x, 0).reshape(70, c, -1).transpose(0, 2, 1)], axis=1)
    assert same_bits(outs[0], (tok + pos[None]).astype(np.float32)) and same_bits(outs[0], outs[1])


# ---- whole models at the project's bar -----------------------------------------------------------------------------------------------------
class TorchViT(torch.nn.Module if torch else object):
    """The float64 twin: nn.Conv2d, class tokens, position table, nn.TransformerEncoder(norm_first, gelu) with its final LayerNorm, nn.Linear."""

    def __init__(self, img, patch, E, h, ff, layers, classes, prefix, seed, w_scale):
        super().__init__()
        torch.manual_seed(seed)
        self.conv = torch.nn.Conv2d(img[0], E, patch, patch)
        S = (img[1] // patch) * (img[2] // patch)
        self.cls = torch.nn.Parameter(0.5 * torch.randn(prefix, E))
        self.pos = torch.nn.Parameter(0.5 * torch.randn(prefix + S, E))
        layer = torch.nn.TransformerEncoderLayer(E, h, ff, dropout=0.0, activation="gelu", batch_first=True, norm_first=True)
        self.enc = torch.nn.TransformerEncoder(layer, layers, norm=torch.nn.LayerNorm(E), enable_nested_tensor=False)
        self.head = torch.nn.Linear(E, classes)
        with torch.no_grad():  # (as torch_encoder(w_scale=...) of tests/test_transformer_gpu.py: every matrix and bias but the norms')
            for name, prm in self.named_parameters():
                if "norm" not in name and name not in ("cls", "pos"):
                    prm.mul_(w_scale)
        self.eval()

    def forward(self, x):
        t = self.conv(x).flatten(2).transpose(1, 2)
        t = torch.cat([self.cls.expand(len(x), -1, -1), t], dim=1) + self.pos
        return self.head(self.enc(t)[:, 0])

    def spec(self, img, patch):
        f = lambda p: p.detach().cpu().numpy().astype(np.float32)  # noqa: E731
        enc = W.from_torch_encoder(self.enc, self.pos.shape[0], head=self.head)
        return {"img": tuple(img), "patch": patch, "E": self.conv.out_channels, "grid": (img[1] // patch, img[2] // patch), "enc": enc,
                "patch_W": f(self.conv.weight), "patch_b": f(self.conv.bias), "cls": f(self.cls), "pos": f(self.pos)}


def run_twin(twin, x, dtype):
    import copy

    with torch.no_grad():
        return copy.deepcopy(twin).to(dtype)(torch.from_numpy(x).to(dtype)).double().numpy()


W_SCALE = 0.25  # torch float32 on the CPU then stays within a quarter of the bar against float64 (asserted below)


@pytest.mark.parametrize("img,prefix", [((3, 16, 16), 1), ((3, 8, 12), 2)], ids=["16x16_cls", "8x12_cls_dist"])
def test_vit_against_torch_float64(api, tmp_path, img, prefix):
    pytest.importorskip("torch")
    twin = TorchViT(img, 4, 32, 4, 64, 2, 5, prefix, seed=11, w_scale=W_SCALE)
    x = np.random.default_rng(5).uniform(-1, 1, (37,) + img).astype(np.float32)
    ref, ref32 = run_twin(twin, x, torch.float64), run_twin(twin, x, torch.float32)
    r32 = worst_ratio(ref32, ref)
    with Served(api, tmp_path, W.vit_from_spec(twin.spec(img, 4))) as m:
        plan = m.api.get_plan(m.name)
        assert [s["kind"] for s in plan["plan"]["steps"]].count("Tokens") == 1 and plan["plan"]["steps"][1]["T"] == prefix + (img[1] // 4) * (img[2] // 4)
        rk = worst_ratio(m(x), ref)
    print(f"\nvit {img} prefix {prefix}: torch-f32 {r32:.4f} kernel {rk:.4f}")
    assert r32 <= 0.25, r32
    assert rk <= 1.0, rk
    # the writer's own float64 restatement agrees with the twin far inside the bar
    assert worst_ratio(W.vit_reference(twin.spec(img, 4), x)["first"], ref) < 1e-3


def test_cnn_stem_encoder_against_torch_float64(api, tmp_path):
    pytest.importorskip("torch")
    spec = W.cnn_stem_encoder_spec(weight_scale=0.5)
    E, enc_spec = spec["E"], spec["enc"]
    torch.manual_seed(3)
    layer = torch.nn.TransformerEncoderLayer(E, enc_spec["h"], enc_spec["ff"], dropout=0.0, activation="relu", batch_first=True, norm_first=False)
    enc = torch.nn.TransformerEncoder(layer, 1, enable_nested_tensor=False).eval()
    head = torch.nn.Linear(E, 4)
    c1, c2 = torch.nn.Conv2d(3, 8, 3, 2, 1), torch.nn.Conv2d(8, E, 3, 2, 1)
    with torch.no_grad():
        for mod in (enc, head, c1, c2):
            for name, prm in mod.named_parameters():
                if "norm" not in name:
                    prm.mul_(0.5)
    f = lambda p: p.detach().numpy().astype(np.float32)  # noqa: E731
    spec.update(W1=f(c1.weight), b1=f(c1.bias), W2=f(c2.weight), b2=f(c2.bias), enc=W.from_torch_encoder(enc, spec["enc"]["T"], head=head))
    pos = torch.from_numpy(spec["pos"])

    def twin(x, dtype):
        with torch.no_grad():
            import copy

            k1, k2, e, hd = (copy.deepcopy(mod).to(dtype) for mod in (c1, c2, enc, head))
            t = k2(torch.relu(k1(torch.from_numpy(x).to(dtype)))).flatten(2).transpose(1, 2) + pos.to(dtype)
            return hd(e(t).mean(dim=1)).double().numpy()

    x = np.random.default_rng(6).uniform(-1, 1, (37, 3, 12, 12)).astype(np.float32)
    ref, r32 = twin(x, torch.float64), None
    r32 = worst_ratio(twin(x, torch.float32), ref)
    with Served(api, tmp_path, W.cnn_stem_encoder_from_spec(spec)) as m:
        rk = worst_ratio(m(x), ref)
    print(f"\ncnn stem + encoder: torch-f32 {r32:.4f} kernel {rk:.4f}")
    assert r32 <= 0.25, r32
    assert rk <= 1.0, rk
    assert worst_ratio(W.cnn_stem_encoder_reference(spec, x)["pooled"], ref) < 1e-3


# ---- call paths, bit-identical ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["step", "step_quads", "vit"])
def test_call_paths_agree(api, tmp_path, which):
    if which == "vit":
        blob, shape = W.vit_from_spec(W.vit_spec(weight_scale=0.25)), (3, 16, 16)
    else:
        blob, shape = W.tokens_model(8, (7, 9), prefix=1, pos=True, front="relu" if which == "step" else "conv")[0], (8, 7, 9)
    x = np.random.default_rng(8).integers(-64, 64, (70,) + shape).astype(np.float32) / 8
    flat = np.ascontiguousarray(x.reshape(70, -1))
    with Served(api, tmp_path, blob, name="paths") as m:
        ref = m(x)
        for i in (0, 33, 69):  # a row alone and inside the batch
            assert same_bits(m(x[i:i + 1]), ref[i]), i
        dev = api.device_ordinal(0)
        d_in, d_out = api.DeviceBuffer(dev, flat.nbytes), api.DeviceBuffer(dev, ref.nbytes)
        d_in.upload(flat)
        api.predict_device("paths", d_in, 70, flat.shape[1], d_out)
        assert same_bits(d_out.download(ref.shape), ref)
        api.predict_device("paths", d_in, 3, flat.shape[1], d_out, in_offset_bytes=20 * flat.shape[1] * 4)  # (rows 20..22 alone, device resident)
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
