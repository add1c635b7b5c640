"""float16 ONNX models without a GPU: the parser's FLOAT16 tensors, the plans of half graphs (HDense steps, the float
path with its RoundHalf steps), what is refused at load, and the numpy reference against torch."""
from __future__ import annotations

import numpy as np
import pytest

from infera_amd import onnx_writer as W


@pytest.fixture(scope="module")
def api(built):
    from infera_amd import capi

    return capi


def load_plan(api, tmp_path, blob, name="h"):
    p = W.write(str(tmp_path / f"{name}.onnx"), blob)
    api.load_model(name, p)
    try:
        return api.get_plan(name)
    finally:
        api.unload_model(name)


def canonical(plan, drop=("origin",)):
    """The steps without their origins, buffers renumbered in the order the steps meet them."""
    ids, out = {0: 0}, []
    for s in plan["plan"]["steps"]:
        s = {k: v for k, v in s.items() if k not in drop}
        for key in ("in", "out"):
            s[key] = ids.setdefault(s[key], len(ids))
        out.append(s)
    return out


def kinds(plan):
    return [s["kind"] for s in plan["plan"]["steps"]]


def special_spec():
    """One 8 -> 4 layer whose weights hold a subnormal, the largest finite halves and both infinities."""
    spec = W.half_mlp_spec((8, 4), seed=5)
    w = spec["layers"][0]["w"]
    w.reshape(-1)[:6] = np.array([0x0001, 0x7BFF, 0xFBFF, 0x7C00, 0xFC00, 0x83FF], np.uint16).view(np.float16)
    return spec


@pytest.mark.parametrize("int32_data", [False, True], ids=["raw_data", "int32_data"])
def test_float16_tensors_round_trip(api, tmp_path, int32_data):
    spec = special_spec()
    plan = load_plan(api, tmp_path, W.half_from_spec(spec, int32_data=int32_data))
    (s,), L = plan["plan"]["steps"], spec["layers"][0]
    bits = L["w"].reshape(-1).view(np.uint16).astype(np.int64)
    assert s["kind"] == "HDense" and (s["K"], s["M"]) == (8, 4)
    assert s["w_sum"] == int(bits.sum()) and s["w_hash"] == int((bits * (np.arange(bits.size) % 251 + 1)).sum())
    assert s["bias_sum"] == int(L["b"].view(np.uint16).astype(np.int64).sum()) and s["bias"] == "gemm"


def test_float16_tensor_whose_bytes_disagree_with_its_dims_is_refused(api, tmp_path):
    spec = W.half_mlp_spec((8, 4), seed=3)
    w = spec["layers"][0]["w"]
    for int32_data in (False, True):
        ok = W.tensor("W0", w, int32_data=int32_data)
        short = W.tensor("W0", w.reshape(-1)[:-1], int32_data=int32_data)
        bad = short.replace(W._vi(1, 31), W._vi(1, 8) + W._vi(1, 4), 1)  # 31 elements under dims [8, 4]
        blob = W.half_from_spec(spec, int32_data=int32_data)
        assert ok in blob
        p = W.write(str(tmp_path / "bad.onnx"), blob.replace(W._ld(5, ok), W._ld(5, bad), 1))
        with pytest.raises(api.InferaError, match="element count does not match dims"):
            api.load_model("bad", p)
    # an odd byte count
    ok = W.tensor("W0", w)
    odd = ok.replace(W._ld(9, w.tobytes()), W._ld(9, w.tobytes() + b"\0"), 1)
    p = W.write(str(tmp_path / "odd.onnx"), W.half_from_spec(spec).replace(W._ld(5, ok), W._ld(5, odd), 1))
    with pytest.raises(api.InferaError, match="element count does not match dims"):
        api.load_model("odd", p)


def test_int32_data_beyond_sixteen_bits_is_refused(api, tmp_path):
    spec = W.half_mlp_spec((8, 4), seed=3)
    w = spec["layers"][0]["w"]
    ok = W.tensor("W0", w, int32_data=True)
    first = int(w.reshape(-1).view(np.uint16)[0])
    wide = ok.replace(W._ld(5, b"".join(W._varint(int(v)) for v in w.reshape(-1).view(np.uint16))),
                      W._ld(5, W._varint(65536) + b"".join(W._varint(int(v)) for v in w.reshape(-1).view(np.uint16)[1:])), 1)
    assert wide != ok, first
    p = W.write(str(tmp_path / "wide.onnx"), W.half_from_spec(spec, int32_data=True).replace(W._ld(5, ok), W._ld(5, wide), 1))
    with pytest.raises(api.InferaError, match="outside the float16 bit patterns"):
        api.load_model("wide", p)


def test_bfloat16_tensor_is_refused_as_before(api, tmp_path):
    spec = W.half_mlp_spec((8, 4), seed=3)
    ok = W.tensor("W0", spec["layers"][0]["w"])
    bf = ok.replace(W._vi(2, W.FLOAT16), W._vi(2, W.BFLOAT16), 1)
    p = W.write(str(tmp_path / "bf.onnx"), W.half_from_spec(spec).replace(W._ld(5, ok), W._ld(5, bf), 1))
    with pytest.raises(api.InferaError, match="unsupported data_type 16"):
        api.load_model("bf", p)


def test_mlp_is_three_hdense_steps_in_every_spelling(api, tmp_path):
    spec = W.half_mlp_spec((128, 256, 64, 1), act="Relu", grid=True)
    plans = {(io, sp): load_plan(api, tmp_path, W.half_from_spec(spec, io=io, spelling=sp)) for io in ("float", "half") for sp in ("gemm", "matmul_add")}
    first = canonical(plans["float", "gemm"], drop=("origin", "bias"))
    for (io, sp), plan in plans.items():
        assert kinds(plan) == ["HDense"] * 3
        assert [(s["K"], s["M"]) for s in plan["plan"]["steps"]] == [(128, 256), (256, 64), (64, 1)]
        assert [s["bias"] for s in plan["plan"]["steps"]] == [sp] * 3 and [s.get("act") for s in plan["plan"]["steps"]] == ["Relu", "Relu", None]
        assert canonical(plan, drop=("origin", "bias")) == first
        assert plan["hdense"] == [{"step": 0, "in": "f32", "out": "half"}, {"step": 1, "in": "half", "out": "half"}, {"step": 2, "in": "half", "out": "f32"}]
        assert plan["plan"].get("input_type") == (None if io == "float" else "float16") and plan["plan"].get("output_type") == (None if io == "float" else "float16")
        assert plan["plan"]["flops_per_row"] == 2 * (128 * 256 + 256 * 64 + 64)


def test_half_edge_knob(api, tmp_path, monkeypatch):
    monkeypatch.setenv("INFERA_HDENSE_HALF", "0")
    plan = load_plan(api, tmp_path, W.half_from_spec(W.half_mlp_spec((128, 256, 64, 1))))
    assert kinds(plan) == ["HDense"] * 3 and all(h["in"] == "f32" and h["out"] == "f32" for h in plan["hdense"])


def test_model_info_names_the_float16_output(api, tmp_path):
    p = W.write(str(tmp_path / "io.onnx"), W.half_from_spec(W.half_mlp_spec((8, 4)), io="half"))
    api.load_model("io", p)
    try:
        assert "float16 output 'Y'" in api.get_model_info("io")["output_served_as"]
    finally:
        api.unload_model("io")


def test_softmax_tail_is_rounded(api, tmp_path):
    plan = load_plan(api, tmp_path, W.half_from_spec(W.half_mlp_spec((30, 100, 2), tail="Softmax")))
    assert kinds(plan) == ["HDense", "HDense", "Softmax", "RoundHalf"]


def test_float_path_switch_and_scaled_gemm(api, tmp_path, monkeypatch):
    spec = W.half_mlp_spec((32, 100, 2))  # (K = 30 would add the float path's PadCols step)
    assert kinds(load_plan(api, tmp_path, W.half_from_spec(spec, alpha=0.5))) == ["RoundHalf", "Dense", "RoundHalf", "Dense", "RoundHalf"]
    monkeypatch.setenv("INFERA_HDENSE", "0")
    assert kinds(load_plan(api, tmp_path, W.half_from_spec(spec))) == ["RoundHalf", "Dense", "RoundHalf", "Dense", "RoundHalf"]
    # MatMul -> Add rounds the product and the sum: two steps, each rounded
    assert kinds(load_plan(api, tmp_path, W.half_from_spec(spec, spelling="matmul_add"))) == ["RoundHalf"] + ["Dense", "RoundHalf", "AffineChannel", "RoundHalf"] * 2


def test_cnn_rounds_behind_convolutions_and_the_average_pool_only(api, tmp_path):
    plan = load_plan(api, tmp_path, W.half_cnn_from_spec(W.half_cnn_spec()))
    # (the first RoundHalf is the Cast of the float input; Relu is fused into the convolutions, MaxPool is exact on halves)
    assert kinds(plan) == ["RoundHalf", "Conv2d", "RoundHalf", "Pool2d", "Conv2d", "RoundHalf", "GlobalAvgPool", "RoundHalf", "HDense"]
    assert [s.get("act") for s in plan["plan"]["steps"] if s["kind"] == "Conv2d"] == ["Relu", "Relu"]


def _two_input_graph(kind):
    h, f = W.FLOAT16, W.FLOAT
    w = np.ones((4, 4), np.float16)
    if kind == "mixed_add":
        nodes = [W.node("Cast", ["X"], ["xh"], [W.attr_i("to", h)]), W.node("MatMul", ["xh", "W"], ["m"]), W.node("Add", ["m", "X"], ["Y"], name="mix")]
    else:
        nodes = [W.node("Cast", ["X"], ["Y"], [W.attr_i("to", W.BFLOAT16)], name="to_bf16")]
    return W.model("bad", nodes, [W.tensor("W", w)], [W.value_info("X", ["N", 4], f)], [W.value_info("Y", ["N", 4], f)])


def test_mixed_types_and_bfloat16_casts_are_refused_by_node(api, tmp_path):
    p = W.write(str(tmp_path / "mix.onnx"), _two_input_graph("mixed_add"))
    with pytest.raises(api.InferaError, match=r"node 'mix' \(Add\): unsupported operator form: it mixes float16 and float activations"):
        api.load_model("mix", p)
    p = W.write(str(tmp_path / "bf.onnx"), _two_input_graph("cast"))
    with pytest.raises(api.InferaError, match=r"node 'to_bf16' \(Cast\)"):
        api.load_model("bf", p)


@pytest.mark.parametrize("spelling", ["gemm", "matmul_add"])
def test_reference_against_torch(spelling):
    torch = pytest.importorskip("torch")
    for grid, dims in ((True, (128, 256, 64, 1)), (True, (30, 100, 2)), (False, (30, 100, 2))):
        spec = W.half_mlp_spec(dims, act="Relu", grid=grid, seed=9)
        x = W.half_inputs(spec, 65, seed=1)
        h = torch.from_numpy(x).half().double()
        for L in spec["layers"]:  # float64 followed by .half()
            acc = h @ torch.from_numpy(L["w"].astype(np.float64))
            b = torch.from_numpy(L["b"].astype(np.float64))
            h = ((acc + b).half() if spelling == "gemm" else (acc.half().double() + b).half()).double()
            if L["act"]:
                h = torch.relu(h)
        want = h.float().numpy()
        got = W.half_reference(spec, x, spelling)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (grid, dims)
        if grid:  # ... and every f32 sum is exact: numpy's own f32 product gives the same bits
            sums = W.half_sums(spec, x, spelling)
            assert all(s < 2.0 ** 24 * q for s, q in zip(sums, spec["q"])), (sums, spec["q"])
            h32 = x.astype(np.float16).astype(np.float32)
            for L in spec["layers"]:
                acc = h32 @ L["w"].astype(np.float32)
                b = L["b"].astype(np.float32)
                h32 = ((acc + b) if spelling == "gemm" else (acc.astype(np.float16).astype(np.float32) + b)).astype(np.float16).astype(np.float32)
                if L["act"]:
                    h32 = np.maximum(h32, 0)
            assert np.array_equal(h32.view(np.uint32), want.view(np.uint32))
