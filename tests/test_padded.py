"""Padded token sequences at load time (no GPU; INTEGRATION.md section 2.6 "Padded sequences"): every spelling of a per-row key mask the
writer knows lowers to ONE Attention step per layer with the expected row_mask object and no step for the mask sub-graph, the masked mean to
ONE MeanTime step; the refusals name their node; graphs without a row mask keep their bytes and their plan; and tests/padded_ref.py agrees
with torch float64 where a row keeps a key and gives the mean of V where it keeps none."""
from __future__ import annotations

import itertools
import json
import os

import numpy as np
import pytest

from infera_amd import onnx_writer as W
from tests import attention_ref as A
from tests import padded_ref as P

FMIN = P.FMIN
NEG_INF = float("-inf")
T, E, H = 16, 32, 2


@pytest.fixture(scope="module")
def api(built):
    from infera_amd import capi

    return capi


def plan_of(api, tmp_path, blob, name="padded", select=""):
    path = W.write(os.path.join(str(tmp_path), name + ".onnx"), blob)
    api.load_model(name, path + select)
    try:
        return api.get_plan(name)
    finally:
        api.unload_model(name)


def load_error(api, tmp_path, blob, name="bad"):
    path = W.write(os.path.join(str(tmp_path), name + ".onnx"), blob)
    with pytest.raises(Exception) as e:
        api.load_model(name, path)
        api.unload_model(name)
    return str(e.value)


def kinds(plan):
    return [s["kind"] for s in plan["plan"]["steps"]]


# ---- every writer form -----------------------------------------------------------------------------------------------------------------

FILLS = [(FMIN, True), (NEG_INF, True), (-10000.0, False), (-1e9, False)]
ADD_FORMS = [dict(form="add", from_ids=ids, unsqueeze=u) for ids in (None, 3) for u in ("one", "two", "reshape")]
REPLACE_FORMS = [dict(form="replace", from_ids=ids, unsqueeze=u, expand=x) for ids in (None, 3) for u in ("one", "two", "reshape") for x in ("none", "const", "shape")]


# ((1 - mask) * -inf is NaN at the kept keys: the additive form has finite fills only, and -inf there is refused: test_refusals_name_their_node)
FORM_CASES = [(kw, fill, ex) for kw in ADD_FORMS + REPLACE_FORMS for fill, ex in FILLS if not (kw["form"] == "add" and fill == NEG_INF)]


@pytest.mark.parametrize("kw,fill,excluding", FORM_CASES, ids=lambda c: "-".join(str(v) for v in c.values()) if isinstance(c, dict) else str(c))
def test_attention_forms_lower_to_one_step(api, tmp_path, kw, fill, excluding):
    p = plan_of(api, tmp_path, W.attention_only(T, E, H, row_mask=dict(kw, fill=fill)))
    assert kinds(p) == ["SliceCols", "Attention"], kinds(p)  # nothing for the mask sub-graph, Expand / Shape included; no SliceCols of M
    att = p["plan"]["steps"][1]
    want = {"src_col": T * 3 * E, "cmp": 0 if kw["from_ids"] is None else 3, "fill": fill, "mode": kw["form"], "excluding": excluding}
    got = dict(att["row_mask"], fill=float(np.float32(att["row_mask"]["fill"])))
    assert got == dict(want, fill=float(np.float32(fill))), (got, want)
    assert att["mask"] is False and att["T"] == T and att["heads"] == H
    assert p["plan"]["input_shape"] == [-1, T * 3 * E + T]


@pytest.mark.parametrize("mask_type", [W.INT64, W.INT32, W.FLOAT], ids=["int64", "int32", "f32"])
def test_mask_input_types(api, tmp_path, mask_type):
    p = plan_of(api, tmp_path, W.attention_only(T, E, H, row_mask=dict(form="add", fill=FMIN), mask_type=mask_type))
    assert kinds(p) == ["SliceCols", "Attention"] and p["plan"]["steps"][1]["row_mask"]["src_col"] == T * 3 * E


@pytest.mark.parametrize("kw", [dict(), dict(form="replace", expand="shape"), dict(form="replace", fill=NEG_INF, from_ids=True, unsqueeze="reshape"),
                                dict(form="add", fill=-10000.0, from_ids=True, unsqueeze="two")], ids=["bert", "distilbert", "ids-replace", "ids-add"])
def test_text_encoder_plan(api, tmp_path, kw):
    spec = W.text_encoder_spec(T=16, V=50, E=32, h=4, ff=64, layers=2)
    blob = W.text_encoder_from_spec(spec, **kw)
    layer = ["Dense", "Attention", "Dense", "BinaryAct", "LayerNorm", "Dense", "Dense", "BinaryAct", "LayerNorm"]
    src = 0 if kw.get("from_ids") else 16
    fill = kw.get("fill", FMIN)
    for select, head in (("#first", ["SliceCols", "Dense"]), ("#sentence", ["MeanTime", "Dense"])):
        p = plan_of(api, tmp_path, blob, select=select)
        assert kinds(p) == ["Embed", "BinaryConst", "LayerNorm"] + layer * 2 + head, kinds(p)  # ONE Attention per layer, the mask computed once
        for s in p["plan"]["steps"]:
            if s["kind"] == "Attention":
                rm = s["row_mask"]
                assert (rm["src_col"], rm["cmp"], rm["mode"], rm["excluding"]) == (src, 0, kw.get("form", "add"), fill <= -1e30), rm
                assert np.float32(rm["fill"]) == np.float32(fill)
            if s["kind"] == "MeanTime":
                assert s["row_mask"]["src_col"] == src and s["row_mask"]["cmp"] == 0 and s["row_mask"]["clip"] == pytest.approx(1e-9, rel=1e-6), s
                assert s["T"] == 16 and s["E"] == 32
        assert p["plan"]["input_shape"] == [-1, 16 if kw.get("from_ids") else 32]


def masked_mean_graph(Tm=7, Em=3, mask_cols=None, **kw):
    nodes, inits = [W.node("Reshape", ["X", "s"], ["x3"])], [W.tensor("s", np.asarray([-1, Tm, Em], np.int64))]
    out = W.masked_mean_nodes(nodes, inits, "mm_", "x3", "M", Tm, Em, **kw)
    return W.model("mm", nodes, inits, [W.value_info("X", ["N", Tm * Em]), W.value_info("M", ["N", mask_cols or Tm], W.INT64)], [W.value_info(out, ["N", Em])], opset=20)


@pytest.mark.parametrize("kw", [dict(), dict(expand="const"), dict(expand="shape", count="mask"), dict(from_ids=2, count="mask", clip=1.0), dict(from_ids=2, expand="shape")],
                         ids=["plain", "expand-const", "expand-shape-count-mask", "ids-clip1", "ids-expand-shape"])
def test_masked_mean_is_one_step(api, tmp_path, kw):
    p = plan_of(api, tmp_path, masked_mean_graph(**kw))
    assert kinds(p) == ["SliceCols", "MeanTime"], kinds(p)
    s = p["plan"]["steps"][1]
    assert s["row_mask"]["src_col"] == 21 and s["row_mask"]["cmp"] == kw.get("from_ids", 0) and s["row_mask"]["clip"] == pytest.approx(kw.get("clip", 1e-9), rel=1e-6)
    assert (s["T"], s["E"]) == (7, 3)


def test_plans_without_a_row_mask_are_unchanged(api, tmp_path):
    """the new writer keywords at their defaults produce the same bytes, and such a plan carries no trace of the feature"""
    spec = W.transformer_spec(T=24, F=8, E=64, h=4, ff=256, layers=2, causal=True)
    pairs = [(W.attention_only(T, E, H), W.attention_only(T, E, H, row_mask=None, mask_type=W.INT64)),
             (W.transformer_from_spec(spec), W.transformer_from_spec(spec, row_mask=None, mean_mask=None))]
    nodes_a, inits_a, nodes_b, inits_b = [], [], [], []
    W.attention_nodes(nodes_a, inits_a, "a_", "q", "k", "v", "q", T, E, H, mask=W.causal_mask(T))
    W.attention_nodes(nodes_b, inits_b, "a_", "q", "k", "v", "q", T, E, H, mask=W.causal_mask(T), row_mask=None)
    assert nodes_a == nodes_b and inits_a == inits_b
    for i, (a, b) in enumerate(pairs):
        assert a == b
        pa, pb = plan_of(api, tmp_path, a, name=f"same{i}a"), plan_of(api, tmp_path, b, name=f"same{i}b")
        sa, sb = json.dumps(pa["plan"], sort_keys=True), json.dumps(pb["plan"], sort_keys=True)
        assert sa == sb and "row_mask" not in sa and "in3" not in sa


# ---- refusals --------------------------------------------------------------------------------------------------------------------------

def custom_attention(build, inputs, form="add", fill=FMIN, mask=None, Tm=T):
    """attention alone over packed X, the row mask's layer-independent value built by `build(nodes, inits)` -> its name"""
    nodes = [W.node("Reshape", ["X", "x_shape"], ["X3"]), W.node("Split", ["X3", "sp"], ["q", "k", "v"], [W.attr_i("axis", 2)], name="split_qkv")]
    inits = [W.tensor("x_shape", np.asarray([-1, Tm, 3 * E], dtype=np.int64)), W.tensor("sp", np.asarray([E, E, E], dtype=np.int64))]
    val = build(nodes, inits)
    out = W.attention_nodes(nodes, inits, "a_", "q", "k", "v", "X3", Tm, E, H, mask=mask, row_mask=dict(form=form, fill=fill, value=val))
    return W.model("attention", nodes, inits, [W.value_info("X", ["N", Tm * 3 * E])] + inputs, [W.value_info(out, ["N", Tm, E])], opset=20)


def i64(name, v):
    return W.tensor(name, np.asarray(v, dtype=np.int64))


def f32(name, v):
    return W.tensor(name, np.asarray(v, dtype=np.float32))


def add_term(nodes, inits, kept4, fill="fill"):
    """(1 - float(kept4)) * fill"""
    inits += [f32("one", 1.0)] + ([f32("fill", FMIN)] if fill == "fill" else [])
    nodes += [W.node("Cast", [kept4], ["kf"], [W.attr_i("to", W.FLOAT)]), W.node("Sub", ["one", "kf"], ["inv"]), W.node("Mul", ["inv", fill], ["term"], name="fill_mul")]
    return "term"


def test_refusals_name_their_node(api, tmp_path):
    err = lambda blob: load_error(api, tmp_path, blob)  # noqa: E731
    M = [W.value_info("M", ["N", T], W.INT64)]

    def unsq(nodes, inits, src="M", axes=(1, 2)):
        inits.append(i64("ax12", list(axes)))
        nodes.append(W.node("Unsqueeze", [src, "ax12"], ["m4"]))
        return "m4"

    # a mask that depends on the query: [N, 1, T, T] out of T * T columns; and on the head too: [N, h, T, T]
    for shape, cols in (([-1, 1, T, T], T * T), ([-1, H, T, T], H * T * T)):
        def per_query(nodes, inits, shape=shape):
            inits.append(i64("s4", shape))
            nodes.append(W.node("Reshape", ["M", "s4"], ["m4"]))
            return add_term(nodes, inits, "m4")
        e = err(custom_attention(per_query, [W.value_info("M", ["N", cols], W.INT64)]))
        assert "node 'a_mask_add' (Add): unsupported operator form:" in e and "depends on the head or the query" in e, e

    # a mask computed from activations
    def from_activation(nodes, inits):
        nodes.append(W.node("Relu", ["Mf"], ["mr"]))
        return add_term(nodes, inits, unsq(nodes, inits, "mr"))
    e = err(custom_attention(from_activation, [W.value_info("Mf", ["N", T])]))
    assert "node 'a_mask_add' (Add): unsupported operator form:" in e and "is not a column range of a graph input" in e and "computed from activations" in e, e

    # a row mask and a constant mask on one attention
    for kw in (dict(form="add", fill=FMIN), dict(form="replace", fill=NEG_INF)):
        e = err(W.attention_only(T, E, H, mask=W.causal_mask(T), row_mask=kw))
        assert ("node 'a_mask_add' (Add)" in e or "node 'a_mask_where' (Where)" in e) and "a row mask and" in e and "on one attention" in e, e

    # the fill: >= 0, NaN, not a scalar, not a constant, -inf in the additive form
    for form in ("add", "replace"):
        node = "node 'a_mask_add' (Add)" if form == "add" else "node 'a_mask_where' (Where)"
        for fill in (0.0, 1.0, float("nan")):
            e = err(W.attention_only(T, E, H, row_mask=dict(form=form, fill=fill)))
            assert node + ": unsupported operator form:" in e and "only a negative number or -inf" in e, e
        e = err(W.attention_only(T, E, H, row_mask=dict(form=form, fill=[-1.0, -2.0])))
        assert node + ": unsupported operator form:" in e and "only one scalar" in e, e
    e = err(W.attention_only(T, E, H, row_mask=dict(form="add", fill=NEG_INF)))
    assert "node 'a_mask_add' (Add): unsupported operator form:" in e and "-inf in the additive form" in e, e

    def variable_fill(nodes, inits):
        inits.append(i64("s1", [-1, 1, 1, 1]))
        nodes.append(W.node("Reshape", ["B", "s1"], ["b4"]))
        return add_term(nodes, inits, unsq(nodes, inits), fill="b4")
    e = err(custom_attention(variable_fill, M + [W.value_info("B", ["N", 1])]))
    assert "node 'a_mask_add' (Add): unsupported operator form:" in e and "is not a constant" in e, e

    # a T that differs from the attention's
    e = err(custom_attention(lambda n, i: add_term(n, i, unsq(n, i)), [W.value_info("M", ["N", T + 1], W.INT64)]))
    assert "node 'a_mask_add' (Add): unsupported operator form:" in e and f"the row mask has T = {T + 1}, the attention T = {T}" in e, e

    # a time-major source
    def time_major(nodes, inits):
        nodes.append(W.node("Transpose", ["M", ], ["mt"], [W.attr_ints("perm", [1, 0])], name="to_rows_first"))
        return add_term(nodes, inits, unsq(nodes, inits, "mt"))
    e = err(custom_attention(time_major, M))
    assert "node 'a_mask_add' (Add): unsupported operator form:" in e and "time-major" in e, e

    # outside the patterns the operators stay unsupported
    nodes = [W.node("Equal", ["X", "c"], ["eq"], name="cmp"), W.node("Cast", ["eq"], ["out"], [W.attr_i("to", W.FLOAT)])]
    e = err(W.model("g", nodes, [f32("c", 0.0)], [W.value_info("X", ["N", 4])], [W.value_info("out", ["N", 4])], opset=20))
    assert "node 'cmp' (Equal)" in e and "unsupported operator" in e, e
    nodes = [W.node("Relu", ["X"], ["r"]), W.node("Greater", ["X", "c"], ["g"], name="gt"), W.node("Where", ["g", "X", "r"], ["out"], name="pick")]
    e = err(W.model("g", nodes, [f32("c", 0.0)], [W.value_info("X", ["N", 4])], [W.value_info("out", ["N", 4])], opset=20))
    assert "unsupported operator" in e, e

    # the masked mean: a T that differs from the window's, a divisor that counts another mask
    e = err(masked_mean_graph(mask_cols=9))
    assert "node 'mm_div' (Div): unsupported operator form:" in e and "the row mask has T = 9, the window T = 7" in e, e


# ---- the reference ---------------------------------------------------------------------------------------------------------------------

def test_reference_agrees_with_torch_float64():
    torch = pytest.importorskip("torch")
    Tq, dh, h, rows = 33, 8, 3, 23
    q, k, v = A.unit_case(Tq, dh * h, rows, seed=3)
    keep = P.keep_rows(Tq, rows)
    sp = lambda a: torch.from_numpy(A.heads_of(a.astype(np.float64), h).copy())  # noqa: E731
    want = torch.nn.functional.scaled_dot_product_attention(sp(q), sp(k), sp(v), attn_mask=torch.from_numpy(keep)[:, None, None, :], scale=0.25)
    want = want.numpy().transpose(0, 2, 1, 3).reshape(rows, Tq, dh * h)
    for mode, fill in (("add", FMIN), ("replace", FMIN), ("replace", NEG_INF), ("add", -1e9)):
        got = P.attention_rows(q, k, v, h, 0.25, keep, fill, mode)
        # (the reference rounds its scores to f32 as the operator does, torch does not: 1e-6 relative, far inside the bar)
        assert P.verdict(got.astype(np.float32), want) <= 0.05, (mode, fill)
        assert np.allclose(got, W.masked_attention_reference(q, k, v, h, keep, fill, mode, scale=0.25), rtol=1e-12, atol=1e-15)


def test_reference_without_a_kept_key():
    Tq, dh, h = 17, 4, 2
    q, k, v = A.unit_case(Tq, dh * h, 3, seed=5)
    keep = np.ones((3, Tq), bool)
    keep[1] = False
    for mode in ("add", "replace"):
        got = P.attention_rows(q, k, v, h, 0.5, keep, FMIN, mode)
        assert np.allclose(got[1], np.broadcast_to(v[1].astype(np.float64).mean(axis=0), (Tq, dh * h)), rtol=1e-13)  # the mean of V over all T keys
        assert np.array_equal(got[[0, 2]], P.attention_rows(q[[0, 2]], k[[0, 2]], v[[0, 2]], h, 0.5, keep[[0, 2]], FMIN, mode))
    assert np.allclose(P.attention_rows(q, k, v, h, 0.5, keep, -1e9, "add")[1], v[1].astype(np.float64).mean(axis=0), rtol=1e-13)
    nan = P.attention_rows(q, k, v, h, 0.5, keep, NEG_INF, "replace")
    assert np.isnan(nan[1]).all() and not np.isnan(nan[[0, 2]]).any()
    x = np.random.default_rng(1).uniform(-1, 1, (3, Tq, 5))
    mm = P.masked_mean(x, keep, 1e-9)
    assert np.array_equal(mm[1], np.zeros(5)) and np.allclose(mm[0], x[0].mean(axis=0), rtol=1e-13)


@pytest.mark.parametrize("fill", [FMIN, -1e9, -10000.0, NEG_INF], ids=["finfo.min", "-1e9", "-1e4", "-inf"])
def test_float32_is_a_fair_case_where_a_key_is_kept(fill):
    """the condition of the GPU cases: with a kept key in every row, the kernel's recurrence in float32 numpy (attention_ref.attention32) sits
    far inside the bar under every fill, so the bar is the kernel's to meet"""
    Tq, dh, h, rows = 48, 16, 2, len(P.PATTERNS)
    q, k, v = A.unit_case(Tq, dh * h, rows, seed=7)
    keep = P.keep_rows(Tq, rows)
    mode = "replace" if fill == NEG_INF else "add"
    ref = P.attention_rows(q, k, v, h, 0.25, keep, fill, mode)
    got = np.stack([A.attention32(q[r:r + 1], k[r:r + 1], v[r:r + 1], h, 0.25, mask=np.where(keep[r], np.float32(0), np.float32(fill)).reshape(1, Tq))[0]
                    for r in range(rows)])
    r32 = P.verdict(got, ref)
    print(f"\nfloat32 recurrence, fill {fill}: {r32:.4f} of the bar")
    assert r32 <= 0.25, r32


def test_patterns_cover_the_tile_edges():
    keep = P.keep_rows(128, len(P.PATTERNS))
    assert keep.any(axis=1).all() and keep[0].all() and keep[1].sum() == 1 and keep[2, -1] and keep[2].sum() == 1
    lengths = sorted(set(int(r.sum()) for r in keep))
    assert {15, 16, 17, 31, 32, 33} <= set(lengths)
    left = keep[P.PATTERNS.index("left17")]
    assert not left[:96].any() and left[-17:].all()  # three wholly masked 32-key tiles, then a partly masked one
    assert not keep[P.PATTERNS.index("tile"), 32:64].any() and keep[P.PATTERNS.index("tile"), :32].all()
    assert list(itertools.islice(keep[P.PATTERNS.index("holes")], 6)) == [True, False, True, True, False, True]
