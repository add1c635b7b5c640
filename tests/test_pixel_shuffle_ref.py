"""The numpy reference of the sub-pixel layers (tests/pixel_shuffle_ref.py) against independent definitions: torch's pixel_shuffle and
pixel_unshuffle on the CPU for the channel-major forms, the specification's reshape / transpose / reshape written out here for the two
block-major forms, and the writer's own pixel_shuffle_apply.  Everything is a copy: the comparisons are bit for bit."""
from __future__ import annotations

import numpy as np
import pytest

from infera_amd import onnx_writer as W

import pixel_shuffle_ref as R

# (form, b, C, H, W)
CASES = [(f, b, (cs * b * b if f in R.TO_SPACE else cs), (h if f in R.TO_SPACE else h * b), (w if f in R.TO_SPACE else w * b))
         for f in R.FORMS for b in (1, 2, 3, 4) for cs in (1, 3, 4) for h, w in ((1, 1), (3, 5))]


def _x(c, h, w, rows=2):
    return R.flat_index_input(rows, (c, h, w))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("form,b,c,h,w", CASES)
def test_index_arrays_are_the_loops(form, b, c, h, w):
    x = _x(c, h, w)
    assert same_bits(R.pixel_shuffle(x, form, b), R.pixel_shuffle_loops(x, form, b))


@pytest.mark.parametrize("form,b,c,h,w", [k for k in CASES if k[0] in ("crd", "unshuffle")])
def test_channel_major_forms_are_torch(form, b, c, h, w):
    import torch
    import torch.nn.functional as F

    x = _x(c, h, w)
    want = (F.pixel_shuffle if form == "crd" else F.pixel_unshuffle)(torch.from_numpy(x), b).numpy()
    assert same_bits(R.pixel_shuffle(x, form, b), want)


@pytest.mark.parametrize("form,b,c,h,w", [k for k in CASES if k[0] in ("dcr", "s2d")])
def test_block_major_forms_are_the_specification(form, b, c, h, w):
    x = _x(c, h, w)
    n = len(x)
    if form == "dcr":  # DepthToSpace, mode DCR, as the operator's specification spells it
        want = x.reshape(n, b, b, c // (b * b), h, w).transpose(0, 3, 4, 1, 5, 2).reshape(n, c // (b * b), h * b, w * b)
    else:  # SpaceToDepth
        want = x.reshape(n, c, h // b, b, w // b, b).transpose(0, 3, 5, 1, 2, 4).reshape(n, c * b * b, h // b, w // b)
    assert same_bits(R.pixel_shuffle(x, form, b), want)


@pytest.mark.parametrize("form,b,c,h,w", CASES)
def test_the_writers_evaluation_is_the_reference(form, b, c, h, w):
    x = _x(c, h, w)
    assert same_bits(W.pixel_shuffle_apply(x, form, b), R.pixel_shuffle(x, form, b))


@pytest.mark.parametrize("up,down", [("dcr", "s2d"), ("crd", "unshuffle")])
@pytest.mark.parametrize("b", [2, 3])
def test_depth_to_space_and_back_is_the_identity(up, down, b):
    x = _x(4 * b * b, 3, 5)
    assert same_bits(R.pixel_shuffle(R.pixel_shuffle(x, up, b), down, b), x)


def test_special_values_keep_their_bits():
    bits = np.array([0x80000000, 0x7F800000, 0xFF800000, 0x7FC00001, 0xFFC12345, 0x00000001, 0x807FFFFF, 0x3F800000], np.uint32)
    x = np.resize(bits, 2 * 16 * 3 * 5).view(np.float32).reshape(2, 16, 3, 5)
    for form in ("dcr", "crd"):
        y = R.pixel_shuffle(x, form, 2)
        assert sorted(y.view(np.uint32).reshape(-1).tolist()) == sorted(x.view(np.uint32).reshape(-1).tolist())


def test_a_bad_shape_is_an_error():
    with pytest.raises(ValueError):
        R.pixel_shuffle(np.zeros((1, 6, 2, 2), np.float32), "crd", 2)
    with pytest.raises(ValueError):
        R.pixel_shuffle(np.zeros((1, 4, 3, 2), np.float32), "s2d", 2)
