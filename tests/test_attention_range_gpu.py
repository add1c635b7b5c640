"""The Transformer kernels (hip/attention.hip: attention_kernel<1, 2, 4, 8>; hip/layernorm.hip: layernorm_kernel<G, NV, VEC>,
mean_time_kernel) through the C ABI against the float64 definitions of tests/attention_ref.py, at the edges tests/test_transformer_gpu.py
does not reach: score ranges of tens to thousands in every key order (the online softmax has to rescale by factors far from 1 and by 0),
queries whose leading sub-tile or whole 32-key tile is -inf, the finite "minus infinities" of exporters, every broadcast shape of the mask,
every head width between the instantiations, every query-tile edge, planted NaN and infinities, every LayerNorm template boundary with
and without B, its input families, and MeanTime's shapes.

Every attention case with large scores has EXACT scores (attention_ref.exact_case), and the fairness rule of the recurrent and encoder
suites holds case by case: a float32 numpy restatement is asserted within a quarter of the bar before the kernel is asserted within it.
Every test asserts from the plan which step served it.  Each case prints its worst error as a share of the bar 1e-4 |ref| + 1e-6 and the
float32 restatement's (profiles/attention_range_ratios.txt holds a run's lines)."""
from __future__ import annotations

import numpy as np
import pytest

from infera_amd import onnx_writer as W
from tests import attention_ref as A

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api(built):
    from infera_amd import capi

    assert capi.device_count() >= 1, capi.get_devices()
    return capi


class Served:
    """one loaded model and its plan"""

    def __init__(self, api, tmp_path, blob, name="attention_range"):
        self.api, self.name = api, name
        api.load_model(name, W.write(str(tmp_path / "m.onnx"), blob))
        self.steps = api.get_plan(name)["plan"]["steps"]
        self.kinds = [s["kind"] for s in self.steps]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.api.unload_model(self.name)

    def rows(self, x):
        return self.api.predict(self.name, np.ascontiguousarray(x.reshape(x.shape[0], -1), np.float32))


def attention_step(m, T, dh, h, mask, scale=None):
    """the plan is ONE Attention step of this geometry (behind the three column cuts of the three-input form)"""
    assert m.kinds in (["Attention"], ["SliceCols"] * 3 + ["Attention"]), m.steps
    s = m.steps[-1]
    assert (s["T"], s["heads"], s["dh"], s["mask"]) == (T, h, dh, mask), s
    if scale is not None:
        assert abs(s["scale"] - scale) <= 1e-5 * scale, s  # (the plan prints six digits; the powers of two exactly)


def default_scale(dh):
    """what the lowering folds Div(scores, f32(sqrt(dh))) into: one f32"""
    return float(np.float32(1.0 / np.float64(np.float32(np.sqrt(dh)))))


def report(site, name, rk, r32=None):
    print(f"{site} {name}: worst error / bar = {rk:.3f}" + ("" if r32 is None else f", float32 = {r32:.3f}"))


def exact_check(m, site, name, q, k, v, h, scale, mask=None):
    """the fairness rule, then the kernel"""
    ref = A.attention(q, k, v, h, scale, mask)
    r32 = A.verdict(A.attention32(q, k, v, h, scale, mask), ref)
    rk = A.verdict(m.rows(A.pack(q, k, v)).reshape(ref.shape), ref)
    report(site, name, rk, r32)
    assert r32 <= 0.25, (site, name, r32)
    assert rk <= 1.0, (site, name, rk)


# ---- attention --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rng_name", list(A.RANGES))
@pytest.mark.parametrize("shape", A.SCORE_SHAPES, ids=lambda c: "T%d_dh%d" % c[:2])
def test_score_range_and_order(api, tmp_path, shape, rng_name):
    """|s| up to about 30, 500 and 16000 (exact), keys random, ascending (the running maximum rises in every 16-key sub-tile: every
    sub-tile rescales o and l, by exactly 0 on the larger ranges), descending (nothing after the first sub-tile survives), and one
    dominant key on either side of each sub-tile and tile edge"""
    T, dh, h, scale = shape
    with Served(api, tmp_path, A.attention_graph(T, dh, h, scale_value=scale)) as m:
        attention_step(m, T, dh, h, False, scale)
        for order in A.score_orders(T):
            q, k, v = A.exact_case(T, dh, h, A.ROWS, rng_name, scale, order)
            exact_check(m, "scores", f"{rng_name} T={T} dh={dh} {order if isinstance(order, str) else 'dominant@%d' % order}", q, k, v, h, scale)


@pytest.mark.parametrize("T", A.MASK_T)
@pytest.mark.parametrize("kind", A.MASK_KINDS)
def test_mask_families(api, tmp_path, kind, T):
    """Bands and left padding: late queries meet a leading sub-tile and a whole leading tile of -inf (the m_new == -inf branch).  -1e9,
    -10000 and finfo.min for -inf, a whole query row of them (accepted at load; uniform weights where f32 absorbs the score), a finite
    ALiBi bias, and the broadcast shapes [1, T], [T], [1, 1, 1, T] (a key mask) and [T, 1] (a per-query bias): the lowering serves each of
    them as the [T, T] table ONNX broadcasting defines (d[0] == 1 ? row 0 : row q, d[1] == 1 ? column 0 : column k)."""
    dh, h, scale = A.MASK_SHAPE
    mask = A.MASKS[kind.replace("-left", "")](T)
    with Served(api, tmp_path, A.attention_graph(T, dh, h, mask=mask, scale_value=scale, mask_left=kind.endswith("-left"))) as m:
        attention_step(m, T, dh, h, True, scale)
        for rng_name in A.MASK_RANGES:
            q, k, v = A.exact_case(T, dh, h, A.ROWS, rng_name, scale, seed=1)
            exact_check(m, "mask", f"{kind} T={T} {rng_name}", q, k, v, h, scale, mask)


@pytest.mark.parametrize("dh,h", [(d, 2) for d in (17, 20, 24, 30, 32, 33, 40, 48, 65, 80, 100, 112, 127)] + [(20, 3)], ids=lambda v: str(v))
def test_head_widths(api, tmp_path, dh, h):
    """attention_kernel<2> (dh 17..32), the padded <4> (33..48) and <8> (65..112, 127), word loads (dh % 4 != 0) and 16-byte loads, head
    offsets that are no multiple of 16 columns; packed [N, T, 3E] and three buffers"""
    T, Em = 33, dh * h
    q, k, v = A.unit_case(T, Em, A.ROWS)
    ref = A.attention(q, k, v, h, default_scale(dh))
    for form in ("packed", "three"):
        with Served(api, tmp_path, A.attention_graph(T, dh, h, form=form)) as m:
            attention_step(m, T, dh, h, False, default_scale(dh))
            rk = A.verdict(m.rows(A.pack(q, k, v, form)).reshape(ref.shape), ref)
        report("widths", f"dh={dh} h={h} {form}", rk)
        assert rk <= 1.0, (form, rk)


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("T", [2, 15, 17, 31, 32, 47, 48, 49, 63, 64, 65, 80, 127, 129])
def test_query_tile_geometry(api, tmp_path, T, causal):
    """1..4 waves, a last wave with one live query (17, 49), a second workgroup along y with one live query and three waves that only
    take part in the barriers (65), key tiles that end on and beside the sub-tile edges"""
    dh, h = 16, 2
    mask = A.causal(T) if causal else None
    q, k, v = A.unit_case(T, dh * h, 19)
    ref = A.attention(q, k, v, h, default_scale(dh), mask)
    with Served(api, tmp_path, A.attention_graph(T, dh, h, mask=mask)) as m:
        attention_step(m, T, dh, h, causal, default_scale(dh))
        rk = A.verdict(m.rows(A.pack(q, k, v)).reshape(ref.shape), ref)
    report("geometry", f"T={T} causal={causal}", rk)
    assert rk <= 1.0, rk


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("where", sorted(A.NONFINITE), ids=lambda w: w[0] + w[1])
def test_nonfinite_inputs(api, tmp_path, where, causal):
    """one NaN / +inf / -inf in Q, K or V of one row and head: the positions attention_ref.NONFINITE derives from the f32 definition, the
    finite rest within the bar, every other head and row bit-identical to the clean run.  The element sits in the second sub-tile
    (key 21) / the second query tile's wave (query 35), and under the causal mask the queries before key 21 give it weight exactly 0."""
    T, dh, h, scale, rows, row, head, i, j, d = 40, 16, 4, 0.25, 5, 2, 1, 35, 21, 3
    mask = A.causal(T) if causal else None
    q, k, v = A.exact_case(T, dh, h, rows, "unit", scale, seed=2)
    bad = {"Q": q.copy(), "K": k.copy(), "V": v.copy()}
    bad[where[0]][row, i if where[0] == "Q" else j, head * dh + d] = A.VALUES[where[1]]
    ref = A.attention(bad["Q"], bad["K"], bad["V"], h, scale, mask)
    nan, inf = A.nonfinite_expectation(A.NONFINITE[where], A.VALUES[where[1]], A.heads_of(q, h)[row, head], mask, i, j, d)
    with Served(api, tmp_path, A.attention_graph(T, dh, h, mask=mask, scale_value=scale)) as m:
        attention_step(m, T, dh, h, causal, scale)
        clean = m.rows(A.pack(q, k, v)).reshape(ref.shape)
        got = m.rows(A.pack(bad["Q"], bad["K"], bad["V"])).reshape(ref.shape)
    mine = A.heads_of(got, h)[row, head]
    assert np.array_equal(np.isnan(mine), nan), (where, np.argwhere(np.isnan(mine) != nan)[:8])
    assert np.array_equal(np.where(np.isinf(mine), mine, 0.0), inf), where
    rk = A.verdict(got, ref)
    report("non-finite", f"{where[0]} {where[1]} causal={causal}", rk)
    assert rk <= 1.0, rk
    keep = np.ones((rows, h), bool)
    keep[row, head] = False
    assert np.array_equal(A.heads_of(got, h)[keep].view(np.uint32), A.heads_of(clean, h)[keep].view(np.uint32)), "another head or row changed"
    assert A.verdict(clean, A.attention(q, k, v, h, scale, mask)) <= 1.0


# ---- LayerNorm --------------------------------------------------------------------------------------------------------------------

def ln_params(E_, seed=0):
    rng = np.random.default_rng([seed, E_])
    return rng.normal(1, 0.2, E_).astype(np.float32), rng.normal(0, 0.2, E_).astype(np.float32)


@pytest.mark.parametrize("E_", A.LN_BOUNDARY_E)
def test_layernorm_template_boundaries(api, tmp_path, E_):
    """both sides of every template boundary (G = 8 / 16 / 32 / 64 lanes, 1 / 4 / 16 quads), 16-byte and word loads, 203 rows so that the
    last block is partly idle ([N, E]: 203 vectors, [N, 5, E]: 1015), with B and without (the beta == nullptr path)"""
    g, b = ln_params(E_)
    for T in (0, 5):
        x = np.random.default_rng([E_, T]).uniform(-1, 1, (203, max(T, 1), E_)).astype(np.float32)
        for bias in (b, None):
            with Served(api, tmp_path, A.layernorm_graph(E_, 1e-5, g, bias, T=T)) as m:
                assert m.kinds == ["LayerNorm"], m.steps
                rk = A.verdict(m.rows(x).reshape(x.shape), A.layernorm(x, g, bias, 1e-5))
            report("layernorm", f"E={E_} {'[N,5,E]' if T else '[N,E]'} {'B' if bias is not None else 'no B'}", rk)
            assert rk <= 1.0, (T, bias is not None, rk)


@pytest.mark.parametrize("E_", A.LN_FAMILY_E)
@pytest.mark.parametrize("family", A.LN_FAMILIES)
def test_layernorm_input_families(api, tmp_path, family, E_):
    """Magnitudes from 1e-18 to 1e15, constant vectors, one outlier, zero and negative gamma, each at eps 1e-12, 1e-5 and 1e-3: the kernel
    within the bar wherever float32 is a fair judge (attention_ref.LN_ASSERTED: torch float32 within a quarter of the bar, measured by
    tests/test_attention_ref.py; the float32 restatement of the documented formula is asserted there too).  Outside the band (a common
    offset of 1e5) only the non-finite pattern is asserted: that of the float32 restatement; the kernel's figure is printed."""
    x, g, b = A.ln_inputs(family, E_)
    for eps in A.LN_EPS:
        ref, r32 = A.layernorm(x, g, b, eps), None
        n32 = A.layernorm32(x, g, b, eps)
        with Served(api, tmp_path, A.layernorm_graph(E_, eps, g, b)) as m:
            assert m.kinds == ["LayerNorm"], m.steps
            got = m.rows(x)
        rk, r32 = A.verdict(got, ref), A.verdict(n32, ref)
        report("layernorm", f"{family} E={E_} eps={eps:g}" + ("" if family in A.LN_ASSERTED else " (outside the band)"), rk, r32)
        if family in A.LN_ASSERTED:
            assert r32 <= 0.25, (eps, r32)
            assert rk <= 1.0, (eps, rk)
        else:
            assert np.array_equal(np.isnan(got), np.isnan(n32)) and np.array_equal(np.isinf(got), np.isinf(n32)), eps


@pytest.mark.parametrize("E_", [33, 768])
def test_layernorm_nan_stays_in_its_vector(api, tmp_path, E_):
    g, b = ln_params(E_)
    x = np.random.default_rng(E_).uniform(-1, 1, (37, 5, E_)).astype(np.float32)
    bad = x.copy()
    bad[3, 2, E_ // 2] = np.nan
    with Served(api, tmp_path, A.layernorm_graph(E_, 1e-5, g, b, T=5)) as m:
        assert m.kinds == ["LayerNorm"], m.steps
        clean, got = m.rows(x).reshape(x.shape), m.rows(bad).reshape(x.shape)
    assert np.isnan(got[3, 2]).all()
    got[3, 2] = clean[3, 2]
    assert np.array_equal(got.view(np.uint32), clean.view(np.uint32)), "a NaN left its vector"
    assert A.verdict(clean, A.layernorm(x, g, b, 1e-5)) <= 1.0


# ---- MeanTime ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("keep", [0, 1])
@pytest.mark.parametrize("T,E_", [(1, 1), (1, 64), (2, 3), (1024, 1), (1024, 5), (100, 257)])
def test_mean_time(api, tmp_path, T, E_, keep):
    """unit inputs and a common offset of 1000 (a running f32 sum of 1024 terms: at most 1024 half-ulp roundings of a partial sum below the
    total, 3e-5 of it against the bar's 1e-4); a NaN, a +inf and a -inf each reach their own column of their own row and nothing else"""
    rows = 211
    u = np.random.default_rng([T, E_]).uniform(-1, 1, (rows, T, E_)).astype(np.float32)
    with Served(api, tmp_path, A.mean_time_graph(T, E_, keep)) as m:
        assert m.kinds == ["MeanTime"], m.steps
        for offset in (0.0, 1000.0):
            x = u + np.float32(offset)
            got = m.rows(x)
            assert got.shape == (rows, E_), got.shape
            rk = A.verdict(got, A.mean_time(x))
            report("mean over time", f"T={T} E={E_} keepdims={keep} offset={offset:g}", rk)
            assert rk <= 1.0, (offset, rk)
        clean, bad = m.rows(u), u.copy()
        planted = [(5, T // 2, 0, np.nan), (100, T - 1, E_ - 1, np.inf), (210, 0, E_ // 2, -np.inf)]
        for r, t, e, val in planted:
            bad[r, t, e] = val
        got = m.rows(bad)
    assert A.verdict(got, A.mean_time(bad)) <= 1.0
    for r, t, e, val in planted:
        assert np.isnan(got[r, e]) if np.isnan(val) else got[r, e] == val, (r, e, got[r, e])
        got[r, e] = clean[r, e]
    assert np.array_equal(got.view(np.uint32), clean.view(np.uint32)), "a non-finite element left its column"
