"""tests/attention_op_ref.py without a GPU: the float64 restatements against torch float64 (scaled_dot_product_attention with is_causal and
enable_gqa, F.rms_norm), and float32 itself (numpy and torch on the CPU) against the float64 restatement on every input family that
tests/test_attention_op_gpu.py asserts at the project's bar -- a family on which float32 arithmetic itself missed the bar would be no fair
case for a float32 kernel."""
from __future__ import annotations

import numpy as np
import pytest

from tests import attention_op_ref as R
from tests import attention_ref as A

torch = pytest.importorskip("torch")
F = torch.nn.functional

# (Tq, Tk, hq, hkv, dh, causal)
TORCH_SHAPES = [(17, 17, 2, 2, 16, True), (33, 33, 4, 2, 16, True), (33, 33, 6, 1, 5, False), (15, 65, 2, 2, 16, True), (33, 17, 4, 2, 16, True),
                (64, 64, 3, 3, 40, True), (1, 33, 2, 1, 64, False)]


def torch_sdpa(q, k, v, hq, hkv, scale, causal, dtype):
    t = lambda a, h: torch.from_numpy(R.heads_of(np.asarray(a), h).copy()).to(dtype)  # noqa: E731
    out = F.scaled_dot_product_attention(t(q, hq), t(k, hkv), t(v, hkv), is_causal=causal, scale=float(scale), enable_gqa=hq != hkv)
    N, Tq = q.shape[0], q.shape[1]
    return out.permute(0, 2, 1, 3).reshape(N, Tq, -1).numpy()


@pytest.mark.parametrize("shape", TORCH_SHAPES, ids=lambda c: "Tq%d_Tk%d_h%d_kv%d_dh%d_%d" % c)
def test_reference_is_torch_float64(shape):
    """exact scores: the two f32 roundings never happen, and the restatement is torch's operator (grouping by repeat_interleave, the causal
    mask aligned top-left) to float64 rounding; uniform inputs: the roundings cost a few 1e-3 of the bar"""
    Tq, Tk, hq, hkv, dh, causal = shape
    worst32 = 0.0
    for kind, bound in (("exact", 1e-6), ("unit", 0.02)):
        q, k, v = R.case(kind, Tq, Tk, hq, hkv, dh, 5, seed=3)
        scale = R.POW2_SCALE[dh]
        ref = R.attention(q, k, v, hq, hkv, scale, causal=causal)
        r = R.verdict(torch_sdpa(q, k, v, hq, hkv, scale, causal, torch.float64).astype(np.float32), ref)
        # (verdict compares a float32 array: the cast costs at most 6e-8 relative, 6e-4 of the bar)
        t64 = torch_sdpa(q, k, v, hq, hkv, scale, causal, torch.float64)
        with np.errstate(all="ignore"):
            direct = float(np.max(np.abs(t64 - ref) / (A.RTOL * np.abs(ref) + A.ATOL)))
        assert direct <= bound, (kind, direct)
        assert r <= 0.02, (kind, r)
        worst32 = max(worst32, R.verdict(torch_sdpa(q, k, v, hq, hkv, scale, causal, torch.float32), ref))
    print(f"\ntorch float32 {shape}: {worst32:.4f} of the bar")
    assert worst32 <= 0.25, worst32


@pytest.mark.parametrize("cfg", R.F64_CASES, ids=R.F64_ID)
def test_float32_is_a_fair_case(cfg):
    """every configuration and input kind of the GPU test's float64 comparison: float32 numpy stays inside a quarter of the bar"""
    Tq, Tk, hq, hkv, dh, causal, padded = cfg
    keep = R.right_padded(R.padded_lengths(Tk), Tk) if padded else None
    for kind in ("unit", "exact"):
        q, k, v = R.case(kind, Tq, Tk, hq, hkv, dh, R.ROWS, seed=1)
        scale = R.POW2_SCALE[dh]
        ref = R.attention(q, k, v, hq, hkv, scale, causal=causal, keep=keep)
        if padded:  # the row that keeps no key has no softmax
            assert np.isnan(ref[0]).all() and not np.isnan(ref[1:]).any()
        r = R.verdict(R.attention32(q, k, v, hq, hkv, scale, causal=causal, keep=keep), ref)
        assert r <= 0.25, (kind, r)


def test_masks_are_the_causal_rule():
    """a bool tril mask, the additive -inf mask and is_causal are one function, also where Tq != Tk"""
    for Tq, Tk in ((17, 17), (15, 33), (33, 17)):
        q, k, v = R.case("unit", Tq, Tk, 4, 2, 16, 3)
        tril = np.tril(np.ones((Tq, Tk), bool))
        a = R.attention(q, k, v, 4, 2, 0.25, causal=True)
        assert np.array_equal(a, R.attention(q, k, v, 4, 2, 0.25, mask=tril))
        assert np.array_equal(a, R.attention(q, k, v, 4, 2, 0.25, mask=np.where(tril, 0.0, -np.inf).astype(np.float32).reshape(1, 1, Tq, Tk)))


def test_grouping_is_repeat_interleave():
    q, k, v = R.case("unit", 9, 9, 6, 2, 5, 3)
    want = R.attention(q, R.repeat_kv(k, 2, 3), R.repeat_kv(v, 2, 3), 6, 6, 0.5)
    assert np.array_equal(R.attention(q, k, v, 6, 2, 0.5), want)


def test_rmsnorm_is_torch_float64():
    for E_ in A.LN_FAMILY_E:
        for eps in A.LN_EPS:
            x, g, _ = R.ln_inputs("scale1e6", E_)
            ref = R.rmsnorm(x, g, eps)
            t = F.rms_norm(torch.from_numpy(x).double(), (E_,), torch.from_numpy(g).double(), float(np.float32(eps))).numpy()
            with np.errstate(all="ignore"):
                assert float(np.max(np.abs(t - ref) / (A.RTOL * np.abs(ref) + A.ATOL))) <= 1e-6


def test_float32_rmsnorm_is_a_fair_case_on_every_family():
    """measured: at most 0.0021 of the bar over LN_FAMILIES x LN_FAMILY_E x LN_EPS, so the GPU test leaves no family out"""
    worst = 0.0
    for fam in A.LN_FAMILIES:
        for E_ in A.LN_FAMILY_E + A.LN_BOUNDARY_E:
            for eps in A.LN_EPS if E_ in A.LN_FAMILY_E else (R.RMS_EPS,):
                x, g, _ = R.ln_inputs(fam, E_)
                worst = max(worst, R.verdict(R.rmsnorm32(x, g, eps), R.rmsnorm(x, g, eps)))
    print(f"\nfloat32 numpy RMSNorm: {worst:.5f} of the bar")
    assert worst <= 0.25, worst
