"""The Rotary step on the GPU (hip/rotary.hip; INTEGRATION.md section 2.6 "Rotary position embeddings").

Same bits: the step alone against the float32 definition of tests/rotary_ref.py over every head width, rotated width, pairing and form the host
selects; Q and K rotated out of a packed projection against the unpacked model; the rotate_half spelling against the operator; a constant
position_ids against tables gathered by hand; special values; one row against the same row among 257.  Against float64 at the project's bar
1e-4 |ref| + 1e-6: Rotary + causal grouped Attention, and the decoder block with rotary against torch float64.  tests/test_rotary_ref.py shows
on the CPU that the float32 definition itself stays within a quarter of the bar on these inputs."""
from __future__ import annotations

import numpy as np
import pytest

from infera_amd import onnx_writer as W
from tests import attention_op_ref as AR
from tests import rotary_ref as R

pytestmark = pytest.mark.gpu

ROWS = R.ROWS


@pytest.fixture(scope="module")
def api(built):
    from infera_amd import capi

    assert capi.device_count() >= 1, capi.get_devices()
    return capi


def run(api, tmp_path, blob, x, name="rotary", plan=None):
    api.load_model(name, W.write(str(tmp_path / f"{name}.onnx"), blob))
    try:
        if plan is not None:
            plan.update(api.get_plan(name)["plan"])
        return api.predict(name, np.ascontiguousarray(x, np.float32).reshape(len(x), -1))
    finally:
        api.unload_model(name)


def run_resident(api, tmp_path, blob, x, name="rotary_resident", plan=None):
    """the device-resident entry: the whole call is ONE pass (the host entry cuts a long call into staging passes of a few thousand rows)"""
    x = np.ascontiguousarray(x, np.float32).reshape(len(x), -1)
    api.load_model(name, W.write(str(tmp_path / f"{name}.onnx"), blob))
    try:
        if plan is not None:
            plan.update(api.get_plan(name)["plan"])
        dev = api.device_ordinal(0)
        d_in, d_out = api.DeviceBuffer(dev, x.nbytes).upload(x), api.DeviceBuffer(dev, x.nbytes)
        api.predict_device(name, d_in, x.shape[0], x.shape[1], d_out)
        return d_out.download(x.shape)
    finally:
        api.unload_model(name)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the step alone: the bits of the float32 definition -----------------------------------------------------------------------------------

def test_the_grid_meets_every_form():
    forms = {(inter, R.expected_form(dh, rd, inter)) for dh, rd, inter, _, _ in R.step_cases()}
    assert forms == {(False, "vec4"), (False, "scalar"), (True, "vec4"), (True, "scalar")}
    assert 36 <= len(R.step_cases()) <= 44
    assert all(R.expected_form(dh, dh, False) == "scalar" for dh in (6, 10))  # an odd dh / 2


@pytest.mark.parametrize("dh,rd,inter,h,T", R.step_cases(), ids=lambda v: str(int(v)))
def test_step_has_the_bits_of_the_definition(api, tmp_path, dh, rd, inter, h, T):
    x = R.inputs("hundred", ROWS, T, h * dh, seed=dh + rd)
    plan = {}
    got = run(api, tmp_path, W.rotary_model(T, h, dh, rotary={"rd": 0 if rd == dh else rd, "interleaved": inter}), x, plan=plan)
    step = plan["steps"][0]
    assert [s["kind"] for s in plan["steps"]] == ["Rotary"] and step["form"] == R.expected_form(dh, rd, inter), step
    assert np.array_equal(bits(got).reshape(x.shape), bits(R.rope32(x, T, h, dh, rd, inter)))


STRIDE = 2048 * 256  # units one pass of the capped grid covers (hip/rotary.hip: kMaxBlocks work groups of kBlock threads)
# (rd, interleaved, form, units per head) at dh = 16: the pair-of-quads form with and without pass-through quads, the quad form with
# and without them, the scalar form in both pairings
STRIDE_CASES = [(16, False, "vec4", 2), (8, False, "vec4", 3), (16, True, "vec4", 4), (4, True, "vec4", 4), (2, False, "scalar", 16), (2, True, "scalar", 16)]


@pytest.mark.parametrize("rd,inter,form,U", STRIDE_CASES)
def test_more_units_than_two_grid_strides(api, tmp_path, rd, inter, form, U):
    """The grid is capped at 2048 work groups of 256 threads and walks the rest of the window with a stride.  6000 rows of T = 33, h = 3,
    dh = 16 in ONE device-resident call hold 6000 x 33 x 3 U units: 2.27 strides at U = 2, 3.4 at U = 3, 4.5 at U = 4 and 18 at U = 16, so
    every form compares values written in its second and later passes.  Neither 3 U nor 33 divides the stride: the unit index carries into
    the vector and the step into T."""
    rows, T, h, dh = 6000, 33, 3, 16
    units = rows * T * h * U
    assert units > 2 * STRIDE and STRIDE % (h * U) != 0 and (STRIDE // (h * U)) % T != 0
    x = R.inputs("unit", rows, T, h * dh, seed=5)
    plan = {}
    got = run_resident(api, tmp_path, W.rotary_model(T, h, dh, rotary={"rd": 0 if rd == dh else rd, "interleaved": inter}), x, plan=plan)
    assert [s["kind"] for s in plan["steps"]] == ["Rotary"]  # (no scratch: the executor runs the call as one pass, one launch)
    assert plan["steps"][0]["form"] == form == R.expected_form(dh, rd, inter)
    want = R.rope32(x, T, h, dh, rd, inter)
    assert np.array_equal(bits(got).reshape(x.shape), bits(want))
    assert not np.array_equal(bits(want[-1]), bits(x[-1]))  # (the last row, written in the last pass, is a rotated one)


# ---- views: Q and K cut from a packed projection ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("h,dh", R.VIEW_SHAPES)
def test_packed_views_have_the_bits_of_the_unpacked_model(api, tmp_path, h, dh):
    T, E = 5, h * dh
    q, k, v = (R.inputs("unit", ROWS, T, E, seed=s) for s in (1, 2, 3))
    plan = {}
    packed = run(api, tmp_path, W.attention_op_model(T, T, h, h, dh, packed=True, rotary=True), np.concatenate([q, k, v], axis=2), plan=plan)
    rots = [s for s in plan["steps"] if s["kind"] == "Rotary"]
    assert [(s["ld"], s["off"]) for s in rots] == [(3 * E, 0), (3 * E, E)] and all(s["form"] == R.expected_form(dh, dh, False, 3 * E, E) for s in rots)
    apart = run(api, tmp_path, W.attention_op_model(T, T, h, h, dh, rotary=True), AR.table(q, k, v))
    assert np.array_equal(bits(packed), bits(apart)) and not np.isnan(packed).any()
    # ... and of the unrotated model over operands rotated by the definition
    by_hand = run(api, tmp_path, W.attention_op_model(T, T, h, h, dh), AR.table(R.rope32(q, T, h, dh), R.rope32(k, T, h, dh), v))
    assert np.array_equal(bits(packed), bits(by_hand))


# ---- spellings -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dh", R.SPELL_DH)
@pytest.mark.parametrize("T", R.SPELL_T)
def test_rotate_half_has_the_bits_of_the_operator(api, tmp_path, T, dh):
    h = R.SPELL_H
    q, k, v = AR.case("unit", T, T, h, h, dh, ROWS, seed=4)
    x = AR.table(q, k, v)
    op = lambda rot: run(api, tmp_path, W.attention_op_model(T, T, h, h, dh, causal=True, scale=AR.POW2_SCALE[dh], rotary=rot), x)  # noqa: E731
    pat = lambda rot: run(api, tmp_path, W.attention_only(T, h * dh, h, form="three", k_transpose="two_step", mask=W.causal_mask(T), scale="scores_mul",  # noqa: E731
                                                          scale_value=AR.POW2_SCALE[dh], rotary=rot, opset=23), x, name="pattern")
    want_op, want_pat = op({"form": "op"}), pat({"form": "op"})
    assert not np.isnan(want_op).any() and np.array_equal(bits(want_op), bits(want_pat))  # is_causal has the bits of the constant mask
    for rot in ({"form": "slice"}, {"form": "split"}, {"form": "slice", "slice_end": "max", "swap": True, "table_rank": 4}):
        assert np.array_equal(bits(op(rot)), bits(want_op)), rot
        assert np.array_equal(bits(pat(rot)), bits(want_pat)), rot
    by_hand = run(api, tmp_path, W.attention_op_model(T, T, h, h, dh, causal=True, scale=AR.POW2_SCALE[dh]), AR.table(R.rope32(q, T, h, dh), R.rope32(k, T, h, dh), v))
    assert np.array_equal(bits(want_op), bits(by_hand))


# ---- positions -------------------------------------------------------------------------------------------------------------------------------

def test_constant_positions_have_the_bits_of_gathered_tables(api, tmp_path):
    T, h, dh, P = 7, 2, 8, 19
    pos = [int(p) for p in np.random.default_rng(3).permutation(P)[:T]]
    x = R.inputs("unit", ROWS, T, h * dh, seed=6)
    got = run(api, tmp_path, W.rotary_model(T, h, dh, rotary={"positions": pos, "cache_rows": P}), x)
    cos, sin = W.rotary_tables(P, dh)
    nodes, inits = [W.node("Reshape", ["X", "s"], ["x3"])], [W.tensor("s", np.asarray([-1, T, h * dh], np.int64))]
    out = W.rotary_op_nodes(nodes, inits, "r_", "x3", cos[pos], sin[pos], num_heads=h)
    by_hand = run(api, tmp_path, W.model("m", nodes, inits, [W.value_info("X", ["N", T * h * dh])], [W.value_info(out, ["N", T, h * dh])], opset=23), x)
    assert np.array_equal(bits(got), bits(by_hand))
    assert np.array_equal(bits(got).reshape(x.shape), bits(R.rope32(x, T, h, dh, positions=pos, cache=R.tables(P, dh))))
    assert not np.array_equal(got, run(api, tmp_path, W.rotary_model(T, h, dh), x))


# ---- values ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dh,rd,inter", [(8, 4, True), (16, 8, False), (6, 2, False), (6, 4, True)])
def test_special_values(api, tmp_path, dh, rd, inter):
    T, h = 5, 3
    x = R.inputs("unit", ROWS, T, h * dh, seed=7).reshape(ROWS, T, h, dh)
    specials = np.array([np.inf, -np.inf, np.nan, -0.0], np.float32)
    for i, sv in enumerate(specials):  # pass-through columns come back as the same bits
        x[i, i % T, i % h, rd + i % (dh - rd)] = sv
    x[4, 2, 1, rd] = np.frombuffer(np.uint32(0x7FC12345).tobytes(), np.float32)[0]  # a NaN with a payload
    blob = W.rotary_model(T, h, dh, rotary={"rd": rd, "interleaved": inter})
    got = run(api, tmp_path, blob, x.reshape(ROWS, -1)).reshape(x.shape)
    assert np.array_equal(bits(got[..., rd:]), bits(x[..., rd:]))
    assert np.array_equal(bits(got), bits(R.rope32(x.reshape(ROWS, T, -1), T, h, dh, rd, inter)).reshape(bits(got).shape))
    assert not np.isnan(got[..., :rd]).any()
    # a NaN in one pair makes exactly that pair NaN
    a, b = (2, 3) if inter else (1, 1 + rd // 2) if rd > 2 else (0, 1)
    x2 = x.copy()
    x2[5, 3, 2, a] = np.nan
    got2 = run(api, tmp_path, blob, x2.reshape(ROWS, -1)).reshape(x.shape)
    hit = np.zeros(x.shape, bool)
    hit[5, 3, 2, a] = hit[5, 3, 2, b] = True
    assert np.isnan(got2[hit]).all() and np.array_equal(bits(got2[~hit]), bits(got[~hit]))


@pytest.mark.parametrize("dh,rd,inter", [(8, 8, False), (6, 6, True)])
def test_one_row_has_the_bits_it_has_among_257(api, tmp_path, dh, rd, inter):
    T, h = 33, 3
    x = R.inputs("unit", 257, T, h * dh, seed=8)
    blob = W.rotary_model(T, h, dh, rotary={"interleaved": inter})
    whole = run(api, tmp_path, blob, x)
    for r in (0, 100, 256):
        assert np.array_equal(bits(run(api, tmp_path, blob, x[r:r + 1])), bits(whole[r:r + 1]))


# ---- against float64, at the project's bar -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("inter", [False, True])
@pytest.mark.parametrize("T", R.PARITY_T)
def test_rotary_and_attention_against_float64(api, tmp_path, T, inter):
    hq, hkv = R.PARITY_HEADS
    dh = R.PARITY_DH
    q, k, v = AR.case("unit", T, T, hq, hkv, dh, ROWS, seed=9)
    ref = AR.attention(R.rope64(q, T, hq, dh, interleaved=inter), R.rope64(k, T, hkv, dh, interleaved=inter), v, hq, hkv, AR.POW2_SCALE[dh], causal=True)
    worst = 0.0
    for form in ("4d", "3d"):
        got = run(api, tmp_path, W.attention_op_model(T, T, hq, hkv, dh, form=form, causal=True, scale=AR.POW2_SCALE[dh], rotary={"interleaved": inter}), AR.table(q, k, v))
        r = R.verdict(got.reshape(ref.shape), ref)
        worst = max(worst, r)
        assert r <= 1.0, (form, r)
    print(f"\nRotary + Attention T={T} interleaved={inter}: {worst:.4f} of the bar")


def torch_rope_decoder(E_, hq, hkv, ff, layers, outputs, T, seed):
    """the decoder of tests/test_attention_op_gpu.py with Hugging Face's apply_rotary_pos_emb on Q and K"""
    import torch

    nn, F = torch.nn, torch.nn.functional
    dh = E_ // hq
    cos, sin = (torch.from_numpy(np.concatenate([t, t], axis=1)) for t in W.rotary_tables(T, dh))

    def rope(t):
        x1, x2 = t[..., : dh // 2], t[..., dh // 2:]
        return t * cos.to(t.dtype) + torch.cat((-x2, x1), dim=-1) * sin.to(t.dtype)

    class Block(nn.Module):
        def __init__(self):
            super().__init__()
            self.norm1, self.norm2 = nn.RMSNorm(E_, eps=1e-6), nn.RMSNorm(E_, eps=1e-6)
            self.q_proj, self.k_proj, self.v_proj = nn.Linear(E_, E_, bias=False), nn.Linear(E_, hkv * dh, bias=False), nn.Linear(E_, hkv * dh, bias=False)
            self.o_proj = nn.Linear(E_, E_, bias=False)
            self.gate, self.up, self.down = nn.Linear(E_, ff, bias=False), nn.Linear(E_, ff, bias=False), nn.Linear(ff, E_, bias=False)

        def forward(self, x):
            N = x.shape[0]
            a = self.norm1(x)
            sp = lambda t, h: t.view(N, T, h, dh).transpose(1, 2)  # noqa: E731
            y = F.scaled_dot_product_attention(rope(sp(self.q_proj(a), hq)), rope(sp(self.k_proj(a), hkv)), sp(self.v_proj(a), hkv), is_causal=True, enable_gqa=True)
            x = x + self.o_proj(y.transpose(1, 2).reshape(N, T, E_))
            f = self.norm2(x)
            return x + self.down(F.silu(self.gate(f)) * self.up(f))

    class Decoder(nn.Module):
        def __init__(self):
            super().__init__()
            self.blocks = nn.ModuleList([Block() for _ in range(layers)])
            self.norm, self.head = nn.RMSNorm(E_, eps=1e-6), nn.Linear(E_, outputs)

        def forward(self, x):
            for b in self.blocks:
                x = b(x)
            return self.head(self.norm(x)[:, -1])

    torch.manual_seed(seed)
    m = Decoder()
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, nn.RMSNorm):
                mod.weight.add_(0.1 * torch.randn(E_))
    return m.eval()


@pytest.mark.parametrize("spelling", ["op", "slice"])
@pytest.mark.parametrize("cfg", [(16, 32, 4, 2, 64), (33, 64, 8, 2, 128)], ids=lambda c: "T%d_E%d_h%d_kv%d_ff%d" % c)
def test_decoder_block_with_rotary_against_torch_float64(api, tmp_path, cfg, spelling):
    import torch

    T, E_, hq, hkv, ff = cfg
    m = torch_rope_decoder(E_, hq, hkv, ff, 2, 3, T, seed=T + E_)
    spec = W.from_torch_decoder_block(m.blocks, m.norm, m.head, T, hq, hkv)
    x = np.random.default_rng(9).uniform(-1, 1, (64, T, E_)).astype(np.float32)
    with torch.no_grad():
        ref = m.double()(torch.from_numpy(x).double()).numpy()
        ref32 = m.float()(torch.from_numpy(x)).numpy()
    assert R.verdict(W.decoder_block_reference(spec, x, rotary=True).astype(np.float32), ref) <= 0.01  # the writer's restatement is torch's model
    r32 = R.verdict(ref32, ref)
    got = run(api, tmp_path, W.decoder_block_from_spec(spec, rotary={"form": spelling}), x.reshape(64, -1), name="decoder")
    rk = R.verdict(got, ref)
    print(f"\ndecoder with rotary {cfg} {spelling}: torch-f32 {r32:.4f} kernel {rk:.4f}")
    assert r32 <= 0.25, r32
    assert rk <= 1.0, rk
