"""The references of tests/rotary_ref.py against independent statements of the rotary embedding, on the CPU: the float64 reference is Hugging
Face's apply_rotary_pos_emb (half pairing) and the complex multiplication (interleaved) in torch float64; the float32 definition is torch
float32's evaluation of the written formula bit for bit; and on the input families of the GPU parity tests the float32 definition stays within
a quarter of the project's bar of float64, so that the bar judges the kernel and not the definition."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from infera_amd import onnx_writer as W
from tests import rotary_ref as R

SHAPES = [(5, 3, 6, 6), (33, 2, 16, 16), (17, 4, 16, 8), (9, 1, 10, 2), (129, 2, 64, 64)]  # T, h, dh, rd


def hf_apply(x4, cos, sin):
    """transformers' apply_rotary_pos_emb on x [N, h, T, dh] with cos, sin [T, dh] (both halves equal)"""
    def rotate_half(t):
        x1, x2 = t[..., : t.shape[-1] // 2], t[..., t.shape[-1] // 2:]
        return torch.cat((-x2, x1), dim=-1)

    return x4 * cos[None, None] + rotate_half(x4) * sin[None, None]


@pytest.mark.parametrize("T,h,dh,rd", SHAPES)
def test_float64_reference_is_hugging_faces_formula(T, h, dh, rd):
    x = R.inputs("unit", 3, T, h * dh, seed=T)
    cos, sin = R.tables(T, rd)
    x4 = torch.from_numpy(x).double().view(3, T, h, dh).transpose(1, 2)
    c, s = (torch.from_numpy(np.concatenate([t, t], axis=1)).double() for t in (cos, sin))
    want = torch.cat([hf_apply(x4[..., :rd], c, s), x4[..., rd:]], dim=-1).transpose(1, 2).reshape(3, T, h * dh).numpy()
    got = R.rope64(x, T, h, dh, rd)
    assert got.dtype == np.float64 and np.array_equal(got, want)


@pytest.mark.parametrize("T,h,dh,rd", SHAPES)
def test_float64_reference_is_the_complex_product_when_interleaved(T, h, dh, rd):
    x = R.inputs("unit", 3, T, h * dh, seed=T + 1)
    cos, sin = R.tables(T, rd)
    x4 = torch.from_numpy(x).double().view(3, T, h, dh)
    z = torch.view_as_complex(x4[..., :rd].reshape(3, T, h, rd // 2, 2).contiguous())
    w = torch.complex(torch.from_numpy(cos).double(), torch.from_numpy(sin).double())[None, :, None, :]
    rot = torch.view_as_real(z * w).reshape(3, T, h, rd)
    want = torch.cat([rot, x4[..., rd:]], dim=-1).reshape(3, T, h * dh).numpy()
    got = R.rope64(x, T, h, dh, rd, interleaved=True)
    # (a complex product may contract a c - b s into one fused operation: equal within two roundings of float64)
    assert np.allclose(got, want, rtol=0, atol=4 * np.finfo(np.float64).eps)


@pytest.mark.parametrize("interleaved", [False, True])
@pytest.mark.parametrize("T,h,dh,rd", SHAPES)
def test_float32_definition_is_torch_float32_bit_for_bit(T, h, dh, rd, interleaved):
    x = R.inputs("hundred", 3, T, h * dh, seed=T + 2)
    Af, Bf = R.factors(*R.tables(T, rd), interleaved)
    j = np.arange(rd)
    partner = (j ^ 1) if interleaved else np.where(j < rd // 2, j + rd // 2, j - rd // 2)
    x4 = torch.from_numpy(x).view(3, T, h, dh)
    a, b = torch.from_numpy(Af)[None, :, None, :], torch.from_numpy(Bf)[None, :, None, :]
    m0, m1 = x4[..., :rd] * a, x4[..., torch.from_numpy(partner)] * b  # two rounded products, one rounded sum
    want = torch.cat([m0 + m1, x4[..., rd:]], dim=-1).reshape(3, T, h * dh).numpy()
    got = R.step32(x, Af, Bf, h, dh, interleaved)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # ... and the writer's restatement is the same function
    assert np.array_equal(W.rotary_reference(x, Af, Bf, h, dh, interleaved).view(np.uint32), got.view(np.uint32))
    assert np.array_equal(W.rotary_reference(x, Af, Bf, h, dh, interleaved, np.float64), R.step64(x, Af, Bf, h, dh, interleaved))


def test_writer_tables_are_the_reference_tables():
    for T, rd in ((1, 2), (33, 16), (129, 64)):
        for got, want in zip(W.rotary_tables(T, rd), R.tables(T, rd)):
            assert got.dtype == np.float32 and np.array_equal(got, want)
    pos = [7, 0, 3]
    assert np.array_equal(W.rotary_tables(3, 8, positions=pos)[1], R.tables(9, 8)[1][pos])
    Af, Bf = W.rotary_factors(*R.tables(5, 6), True)
    assert np.array_equal(Af, R.factors(*R.tables(5, 6), True)[0]) and np.array_equal(Bf, R.factors(*R.tables(5, 6), True)[1])
    Af, Bf = W.rotary_factors(*R.tables(5, 6), False)
    assert np.array_equal(Af, R.factors(*R.tables(5, 6), False)[0]) and np.array_equal(Bf, R.factors(*R.tables(5, 6), False)[1])


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("interleaved", [False, True])
def test_float32_definition_is_within_a_quarter_of_the_bar(family, interleaved):
    worst = 0.0
    for T, h, dh, rd in SHAPES + [(t, R.PARITY_HEADS[0], R.PARITY_DH, R.PARITY_DH) for t in R.PARITY_T]:
        x = R.inputs(family, 64, T, h * dh, seed=T)
        worst = max(worst, R.verdict(R.rope32(x, T, h, dh, rd, interleaved), R.rope64(x, T, h, dh, rd, interleaved)))
    print(f"\nfloat32 definition, {family}, interleaved={interleaved}: {worst:.4f} of the bar")
    assert worst <= 0.25, worst
