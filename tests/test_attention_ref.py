"""tests/attention_ref.py checked without a GPU: the float64 attention against the writer's plain restatement where the two definitions
coincide, the rounded-score rule on the finite "minus infinities", exact scores and the float32 restatement's share of the bar on every
exact-score case of tests/test_attention_range_gpu.py (the fairness rule: <= 0.25), the non-finite table against the literal IEEE
evaluation, the LayerNorm band against torch float32, and what the lowering makes of every mask the GPU file serves."""
from __future__ import annotations

import numpy as np
import pytest

from infera_amd import onnx_writer as W
from tests import attention_ref as A


def test_reference_agrees_with_the_plain_restatement():
    """exact scores, -inf masks: no rounding separates the two definitions"""
    q, k, v = A.exact_case(33, 16, 2, 3, "unit", 0.25)
    for mask in (None, A.causal(33), A.banded(33, 3)):
        got, want = A.attention(q, k, v, 2, 0.25, mask), W.attention_reference(q, k, v, 2, scale=0.25, mask=mask)
        assert np.allclose(got, want, rtol=1e-12, atol=1e-14)
    x = np.random.default_rng(0).uniform(-1, 1, (5, 7, 33)).astype(np.float32)
    g, b = np.linspace(0.5, 1.5, 33, dtype=np.float32), np.linspace(-1, 1, 33, dtype=np.float32)
    assert np.allclose(A.layernorm(x, g, b, 1e-5), W.layernorm_reference(x, g, b, np.float32(1e-5)), rtol=1e-12, atol=1e-14)
    assert np.array_equal(A.mean_time(x), x.astype(np.float64).sum(1) / 7)


def test_rounded_score_rule():
    """a query masked by -1e9 at every key has uniform weights where |s| < 32 (fl32 absorbs the score), by finfo.min always; a causal mask
    spelled -1e9 / finfo.min is the -inf one to the last bit of the weights that survive"""
    T = 33
    q, k, v = A.exact_case(T, 16, 2, 3, "unit", 0.25)
    assert np.abs(A.scores64(q, k, 2, 0.25)).max() < 32
    uniform = A.heads_of(v.astype(np.float64), 2).mean(axis=2)  # [N, h, dh]
    for fill in (-1e9, A.FMIN):
        out = A.heads_of(A.attention(q, k, v, 2, 0.25, A.full_row(T, fill)), 2)
        assert np.allclose(out[:, :, T // 2], uniform, rtol=1e-13, atol=1e-15)
        assert np.allclose(A.attention(q, k, v, 2, 0.25, A.causal(T, fill)), A.attention(q, k, v, 2, 0.25, A.causal(T)), rtol=1e-13, atol=1e-15)
    qw, kw, vw = A.exact_case(T, 16, 2, 3, "huge", 0.25)
    out = A.heads_of(A.attention(qw, kw, vw, 2, 0.25, A.full_row(T, A.FMIN)), 2)
    assert np.allclose(out[:, :, T // 2], A.heads_of(vw.astype(np.float64), 2).mean(axis=2), rtol=1e-13, atol=1e-15)
    s = A.rounded_scores(qw, kw, 2, 0.25, A.full_row(T, -1e9))[:, :, T // 2]
    assert (s % 64 == 0).all() and len(np.unique(s)) > 1  # thousands survive -1e9 in steps of 64: not uniform, and well defined


@pytest.mark.parametrize("rng_name", list(A.RANGES))
@pytest.mark.parametrize("shape", A.SCORE_SHAPES, ids=lambda c: "T%d_dh%d" % c[:2])
def test_score_cases_are_exact_and_fair(rng_name, shape):
    """exact_case() asserts exactness, the rising maximum and the dominant key itself"""
    T, dh, h, scale = shape
    for order in A.score_orders(T):
        q, k, v = A.exact_case(T, dh, h, A.ROWS, rng_name, scale, order)
        r32 = A.verdict(A.attention32(q, k, v, h, scale), A.attention(q, k, v, h, scale))
        assert r32 <= 0.25, (order, r32)


@pytest.mark.parametrize("kind", A.MASK_KINDS)
def test_mask_cases_are_fair(kind):
    dh, h, scale = A.MASK_SHAPE
    for T in A.MASK_T:
        mask = A.MASKS[kind.replace("-left", "")](T)
        tt = A.mask_tt(mask, T)
        if kind in A.INF_KINDS and (T >= 65 or kind == "leftpad"):  # some query meets an all -inf leading sub-tile / 32-key tile
            assert np.isneginf(tt[:, :16]).all(axis=1).any() and np.isneginf(tt[:, :32]).all(axis=1).any()
        for rng_name in A.MASK_RANGES:
            q, k, v = A.exact_case(T, dh, h, A.ROWS, rng_name, scale, seed=1)
            ref = A.attention(q, k, v, h, scale, mask)
            assert np.isfinite(ref).all()
            r32 = A.verdict(A.attention32(q, k, v, h, scale, mask), ref)
            assert r32 <= 0.25, (T, rng_name, r32)


@pytest.mark.parametrize("mask", [None, "causal"])
@pytest.mark.parametrize("where", sorted(A.NONFINITE))
def test_nonfinite_table_is_the_ieee_evaluation(where, mask):
    """NONFINITE against attention() itself, which forms every product: NaN and infinity positions, and every other head and row
    unchanged to the bit"""
    T, dh, h, row, head, i, j, d = 33, 16, 4, 2, 1, 9, 5, 3
    mk = A.causal(T) if mask else None
    q, k, v = A.exact_case(T, dh, h, 5, "unit", 0.25, seed=2)
    clean = A.attention(q, k, v, h, 0.25, mk)
    bad = {"Q": q.copy(), "K": k.copy(), "V": v.copy()}
    bad[where[0]][row, i if where[0] == "Q" else j, head * dh + d] = A.VALUES[where[1]]
    got = A.attention(bad["Q"], bad["K"], bad["V"], h, 0.25, mk)
    nan, inf = A.nonfinite_expectation(A.NONFINITE[where], A.VALUES[where[1]], A.heads_of(q, h)[row, head], mk, i, j, d)
    mine = A.heads_of(got, h)[row, head]
    assert np.array_equal(np.isnan(mine), nan) and np.array_equal(np.where(np.isinf(mine), mine, 0.0), inf)
    if A.NONFINITE[where] == "head-by-sign":
        assert nan.any() and not nan.all()  # the case shows both signs
    keep = np.ones((5, h), bool)
    keep[row, head] = False
    assert np.array_equal(A.heads_of(got, h)[keep], A.heads_of(clean, h)[keep])


def test_layernorm_band_against_torch_float32():
    """The asserted families are those where torch float32 layer_norm is within a quarter of the bar of float64; the family outside
    (a common offset of 1e5: torch's single-pass variance) is compared by its non-finite pattern only."""
    torch = pytest.importorskip("torch")
    for family in A.LN_FAMILIES:
        for eps in A.LN_EPS:
            for E_ in A.LN_FAMILY_E:
                x, g, b = A.ln_inputs(family, E_)
                ref = A.layernorm(x, g, b, eps)
                t = torch.nn.functional.layer_norm(torch.from_numpy(x), (E_,), torch.from_numpy(g), torch.from_numpy(b), eps).numpy()
                r32 = A.verdict(t, ref)
                assert (r32 <= 0.25) == (family in A.LN_ASSERTED), (family, eps, E_, r32)
                assert np.isfinite(A.layernorm32(x, g, b, eps)).all()


def test_lowering_of_every_mask(tmp_path, built):
    """every mask kind and shape of the GPU file is accepted at load and lowers to ONE Attention step with the mask flag set"""
    from infera_amd import capi

    T = 33
    dh, h, scale = A.MASK_SHAPE
    for n, kind in enumerate(A.MASK_KINDS):
        blob = A.attention_graph(T, dh, h, mask=A.MASKS[kind.replace("-left", "")](T), scale_value=scale, mask_left=kind.endswith("-left"))
        capi.load_model(f"mk{n}", W.write(str(tmp_path / f"mk{n}.onnx"), blob))
        try:
            steps = capi.get_plan(f"mk{n}")["plan"]["steps"]
        finally:
            capi.unload_model(f"mk{n}")
        assert [s["kind"] for s in steps] == ["Attention"], (kind, steps)
        assert steps[0]["mask"] is True and steps[0]["scale"] == scale and (steps[0]["T"], steps[0]["heads"], steps[0]["dh"]) == (T, h, dh), (kind, steps)
