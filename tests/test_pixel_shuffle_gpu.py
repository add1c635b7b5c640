"""DepthToSpace, SpaceToDepth and their spellings on the GPU (INTEGRATION.md 2.6 "Sub-pixel layers"), through predict_from_blob on 1, 3 and 70
rows.  The step only copies, so everything about it is compared BIT FOR BIT with the index-formula reference (tests/pixel_shuffle_ref.py): every
form crossed with the block sizes, channel counts, plane sizes and layout pairings at which the kernel takes another path, the kernel form the
plan names asserted per case; special values as uint32; the bit identities (a spelling and its operator, depth to space and back, a row alone
and in its batch, a fast form and the generic form).  The input values are the elements' own flat indices, so a wrong source names itself.  The
ESPCN and stem models are checked against their float64 evaluation at the project's parity bar: the convolutions carry that error."""
from __future__ import annotations

import numpy as np
import pytest

from infera_amd import onnx_writer as W

import pixel_shuffle_ref as R

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 1e-6
ROWS = (1, 3, 70)
CQ, NCHW = "NC/4HW4", "NCHW"
FORM_NAMES = {"dcr": "depth_to_space_dcr", "crd": "depth_to_space_crd", "s2d": "space_to_depth", "unshuffle": "pixel_unshuffle"}
# how the layer under test is embedded: identity 1x1 layers around it put it on channel-quad tensors (the model's own input and a served
# [C,H,W] result are NCHW); "stem": it reads the caller's image and writes channel quads
EMBEDDINGS = {"cq_in_cq_out": dict(pre=True, post=True), "cq_in_nchw_out": dict(pre=True, post=False), "nchw_in_nchw_out": dict(pre=False, post=False),
              "nchw_in_cq_out": dict(pre=False, post=True)}


@pytest.fixture(scope="module")
def api(built):
    from infera_amd import capi

    assert capi.device_count() >= 1, capi.get_devices()
    return capi


class Served:
    def __init__(self, api, tmp_path, blob, name="ps"):
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


def serve(api, tmp_path, monkeypatch, blob, fast=True, name="ps"):
    if fast:
        monkeypatch.delenv("INFERA_PIXELSHUFFLE_FAST", raising=False)
    else:
        monkeypatch.setenv("INFERA_PIXELSHUFFLE_FAST", "0")  # (read when a model is loaded)
    return Served(api, tmp_path, blob, name)


def same_bits(got, want):
    got, want = np.ascontiguousarray(got, np.float32).reshape(-1), np.ascontiguousarray(want, np.float32).reshape(-1)
    return got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def first_difference(got, want):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    return None if not len(bad) else (int(bad[0]), float(got[bad[0]]), float(want[bad[0]]), len(bad))


def in_dims(form, b, cs, hw):
    """the input (C, (H, W)) of a layer whose spatially larger side is [cs, hw * b]"""
    return (cs * b * b, hw) if form in R.TO_SPACE else (cs, (hw[0] * b, hw[1] * b))


def expected(form, b, c, hw, pre, post, fast=True):
    """(kernel, in_layout, out_layout): the scheduler's rules, restated.  An internal [N,C,H,W] tensor needs whole quads for the plan to be in
    channel quads (a [N,C,1,1] one without them is plain instead); the caller's image and a served [C,H,W] result are NCHW."""
    oc, oh, ow = R.out_shape(form, b, c, *hw)
    internal = ([(c, hw[0] * hw[1])] if pre else []) + ([(oc, oh * ow)] if post else [])
    cq_mode = (pre or post) and all(ch % 4 == 0 or sp == 1 for ch, sp in internal)
    in_cq = cq_mode and pre and c % 4 == 0
    out_cq = cq_mode and oc % 4 == 0 and (post or oh * ow == 1)
    small = oc if form in R.TO_SPACE else c
    if not fast or (not in_cq and not out_cq):
        kernel = "pixelshuffle_generic"
    elif in_cq and out_cq:
        block_major = form in ("dcr", "s2d")
        kernel = "pixelshuffle_quad_copy" if block_major and small % 4 == 0 else "pixelshuffle_transpose" if not block_major and b in (2, 4) else "pixelshuffle_generic"
    else:
        kernel = "pixelshuffle_cq_to_nchw" if in_cq else "pixelshuffle_nchw_to_cq"
    return kernel, (CQ if in_cq else NCHW), (CQ if out_cq else NCHW)


def check_layer(api, tmp_path, monkeypatch, form, b, cs, hw, emb, rows=ROWS):
    c, ihw = in_dims(form, b, cs, hw)
    blob, spec = W.pixel_shuffle_model(form, b, c, ihw, spelling=form == "unshuffle", **EMBEDDINGS[emb])
    want_kernel = expected(form, b, c, ihw, **EMBEDDINGS[emb])
    outs = {}
    with serve(api, tmp_path, monkeypatch, blob) as m:
        k = m.plan["pixelshuffle"][0]
        assert (k["kernel"], k["in_layout"], k["out_layout"]) == want_kernel and (k["form"], k["block"]) == (FORM_NAMES[form], b), (k, want_kernel)
        for n in rows:
            x = R.flat_index_input(n, (c,) + tuple(ihw))
            outs[n] = m(x)
            assert same_bits(outs[n], R.pixel_shuffle(x, form, b)), (n, first_difference(outs[n], R.pixel_shuffle(x, form, b)))
    if want_kernel[0] != "pixelshuffle_generic":  # the fast form against the generic form on the same model
        with serve(api, tmp_path, monkeypatch, blob, fast=False) as m:
            k = m.plan["pixelshuffle"][0]
            assert (k["kernel"], k["in_layout"], k["out_layout"]) == ("pixelshuffle_generic",) + want_kernel[1:], k
            for n in rows:
                assert same_bits(m(R.flat_index_input(n, (c,) + tuple(ihw))), outs[n]), n
    return want_kernel[0]


PLANES = [(1, 1), (3, 5)]
BLOCKS = [2, 3, 4]
# (embedding, the channel counts of the spatially larger side): whole quads and two of them on channel-quad tensors; 1 and 3 where only the
# served output holds them; 5 in NCHW throughout; the stem's 3 (an image) and 4
CHANNELS = {"cq_in_cq_out": (4, 8), "cq_in_nchw_out": (1, 3, 4), "nchw_in_nchw_out": (5,), "nchw_in_cq_out": (3, 4)}
CASES = [pytest.param(form, b, cs, hw, emb, id=f"{form}-b{b}-c{cs}-{hw[0]}x{hw[1]}-{emb}") for emb in EMBEDDINGS for form in R.FORMS for b in BLOCKS
         for cs in CHANNELS[emb] for hw in PLANES]


@pytest.mark.parametrize("form,b,cs,hw,emb", CASES)
def test_every_form_block_and_layout_is_the_reference(api, tmp_path, monkeypatch, form, b, cs, hw, emb):
    check_layer(api, tmp_path, monkeypatch, form, b, cs, hw, emb)


def test_the_cases_reach_every_kernel_form():
    """the shapes above were chosen so that each form of the kernel runs, in both directions where it has two"""
    seen = {}
    for p in CASES:
        form, b, cs, hw, emb = p.values
        c, ihw = in_dims(form, b, cs, hw)
        seen.setdefault(expected(form, b, c, ihw, **EMBEDDINGS[emb])[0], set()).add((form, b))
    assert set(seen) == {"pixelshuffle_generic", "pixelshuffle_quad_copy", "pixelshuffle_transpose", "pixelshuffle_cq_to_nchw", "pixelshuffle_nchw_to_cq"}
    assert {("crd", 2), ("crd", 4), ("unshuffle", 2), ("unshuffle", 4)} <= seen["pixelshuffle_transpose"]
    assert {("dcr", 3), ("s2d", 3)} <= seen["pixelshuffle_quad_copy"]
    assert {("crd", 2), ("crd", 4), ("dcr", 2), ("s2d", 2)} <= seen["pixelshuffle_cq_to_nchw"]
    assert {("unshuffle", 2), ("s2d", 2), ("crd", 2)} <= seen["pixelshuffle_nchw_to_cq"]


def test_more_than_one_workgroup_and_a_partial_one(api, tmp_path, monkeypatch):
    """70 rows of 32 -> 8 channels on 7 x 9: 4410 quads per form and more, several workgroups and a last partial one, on each fast form"""
    for form, emb in (("crd", "cq_in_cq_out"), ("dcr", "cq_in_cq_out"), ("unshuffle", "cq_in_cq_out"), ("crd", "cq_in_nchw_out"), ("unshuffle", "nchw_in_cq_out")):
        assert check_layer(api, tmp_path, monkeypatch, form, 2, 8, (7, 9), emb, rows=(70,)) != "pixelshuffle_generic"


def test_special_values_keep_their_bits(api, tmp_path, monkeypatch):
    """-0, +-inf, NaNs with payloads, subnormals: compared as uint32 (no convolution in these plans: the values reach the step untouched)"""
    bits = np.array([0x80000000, 0x7F800000, 0xFF800000, 0x7FC00001, 0xFFC12345, 0x00000001, 0x807FFFFF, 0x3F800000, 0x00000000], np.uint32)
    for form, c, hw in (("crd", 16, (3, 5)), ("dcr", 16, (3, 5)), ("unshuffle", 4, (6, 10)), ("s2d", 4, (6, 10))):
        blob, _ = W.pixel_shuffle_model(form, 2, c, hw, spelling=form == "unshuffle")
        x = np.resize(bits, 3 * c * hw[0] * hw[1]).view(np.float32).reshape((3, c) + hw)
        with serve(api, tmp_path, monkeypatch, blob) as m:
            got = m(x)
        assert same_bits(got, R.pixel_shuffle(x, form, 2)), form


@pytest.mark.parametrize("form", ["dcr", "crd", "s2d"])
@pytest.mark.parametrize("emb", ["cq_in_cq_out", "cq_in_nchw_out"])
def test_a_spelling_is_its_operator(api, tmp_path, monkeypatch, form, emb):
    c, hw = in_dims(form, 2, 4, (3, 5))
    x = R.flat_index_input(3, (c,) + hw)
    outs = []
    for kw in (dict(), dict(spelling=True), dict(spelling=True, target="shape", lead=-1)):
        with serve(api, tmp_path, monkeypatch, W.pixel_shuffle_model(form, 2, c, hw, **EMBEDDINGS[emb], **kw)[0]) as m:
            outs.append(m(x))
    assert same_bits(outs[1], outs[0]) and same_bits(outs[2], outs[0])


@pytest.mark.parametrize("emb", ["cq_in_cq_out", "nchw_in_nchw_out"])
@pytest.mark.parametrize("b", [2, 3])
@pytest.mark.parametrize("form", ["dcr", "crd"])
def test_depth_to_space_and_back_is_the_input(api, tmp_path, monkeypatch, form, b, emb):
    c, hw = 4 * b * b, (3, 5)
    blob, _ = W.pixel_shuffle_pair_model(form, b, c, hw, **EMBEDDINGS[emb])
    with serve(api, tmp_path, monkeypatch, blob) as m:
        assert [k["form"] for k in m.plan["pixelshuffle"]] == [FORM_NAMES[form], FORM_NAMES["s2d" if form == "dcr" else "unshuffle"]]
        for n in ROWS:
            x = R.flat_index_input(n, (c,) + hw)
            assert same_bits(m(x), x), n


@pytest.mark.parametrize("form,emb", [("crd", "cq_in_cq_out"), ("dcr", "cq_in_nchw_out"), ("s2d", "nchw_in_nchw_out"), ("unshuffle", "nchw_in_cq_out")])
def test_a_row_alone_is_the_row_in_its_batch(api, tmp_path, monkeypatch, form, emb):
    c, hw = in_dims(form, 2, 4, (3, 5))
    blob, _ = W.pixel_shuffle_model(form, 2, c, hw, spelling=form == "unshuffle", **EMBEDDINGS[emb])
    x = R.flat_index_input(70, (c,) + hw)
    with serve(api, tmp_path, monkeypatch, blob) as m:
        whole = m(x)
        for r in (0, 1, 37, 69):
            assert same_bits(m(x[r:r + 1]), whole[r:r + 1]), r


# ---- the models -------------------------------------------------------------------------------------------------------------------------
def within_parity(got, want):
    want = np.asarray(want, np.float64).reshape(len(got), -1)
    excess = np.abs(got.astype(np.float64) - want) - (RTOL * np.abs(want) + ATOL)
    return float(excess.max()) <= 0.0, float(np.abs(got - want).max())


@pytest.mark.parametrize("spelling", [False, True], ids=["op", "spelling"])
@pytest.mark.parametrize("b", [2, 4])
def test_espcn_against_float64(api, tmp_path, monkeypatch, b, spelling):
    blob, spec = W.espcn(b=b, spelling=spelling)
    rng = np.random.default_rng(7)
    with serve(api, tmp_path, monkeypatch, blob) as m:
        k = m.plan["pixelshuffle"][0]
        assert m.plan["activation_layout"] == CQ and (k["in_layout"], k["out_layout"], k["kernel"]) == (CQ, NCHW, "pixelshuffle_cq_to_nchw"), k
        for n in ROWS:
            x = rng.uniform(-1, 1, size=(n,) + tuple(spec["in_shape"])).astype(np.float32)
            ok, err = within_parity(m(x), W.decoder_reference(spec, x))
            assert ok, (n, err)


@pytest.mark.parametrize("b", [2, 4])
def test_stem_against_float64(api, tmp_path, monkeypatch, b):
    blob, spec = W.pixel_unshuffle_stem(b=b)
    rng = np.random.default_rng(9)
    with serve(api, tmp_path, monkeypatch, blob) as m:
        k = m.plan["pixelshuffle"][0]
        assert m.plan["activation_layout"] == CQ and (k["in_layout"], k["out_layout"], k["kernel"]) == (NCHW, CQ, "pixelshuffle_nchw_to_cq"), k
        for n in ROWS:
            x = rng.uniform(-1, 1, size=(n,) + tuple(spec["in_shape"])).astype(np.float32)
            ok, err = within_parity(m(x), W.decoder_reference(spec, x))
            assert ok, (n, err)
