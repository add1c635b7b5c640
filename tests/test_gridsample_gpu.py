"""GridSample and AffineGrid on the GPU (INTEGRATION.md 2.6 "Grid sampling"), through predict_from_blob: 5 x 7 images sampled to 6 x 11, three
images per call (66 positions each, so a wave's 64 positions straddle images) and five (two work groups, the last one partial).  Every result
is compared BIT FOR BIT with the float32 restatement of the contract (tests/gridsample_ref.py) and, within the bound test_gridsample_ref.py
records, with float64 torch.  On NCHW the coordinates are a second input of the call; on channel quads (identity 1x1 layers around the step)
they are constants a zero-weight localisation net hands to every image, and the pixels are multiples of 2^-8, which those layers pass on
exactly.  The edge-value case was run only after tests/native/gridsample_index (the same coordinate function under host sanitizers) was clean."""
from __future__ import annotations

import itertools

import numpy as np
import pytest

from infera_amd import onnx_writer as W

import gridsample_ref as R
from test_gridsample_ref import HW, MARGIN, OUT_HW

pytestmark = pytest.mark.gpu
CQ, NCHW = "NC/4HW4", "NCHW"
COMBOS = list(itertools.product(R.MODES, R.PADDINGS, R.ALIGNS))
# five warps (shears, rotations, shrinks, some beyond the image) whose grids keep 2^-10 from every tie at these extents: check() asserts it
THETAS = np.array([[1.427, 0.468, -0.485, 0.364, 1.481, 0.457], [1.388, -0.274, -0.375, -0.212, 1.086, 0.054], [1.459, -0.131, 0.053, 0.094, 1.348, -0.355],
                   [0.51, -0.135, -0.421, 0.153, 0.774, 0.203], [1.478, 0.09, -0.18, -0.312, 1.173, -0.305]], np.float32)


@pytest.fixture(scope="module")
def api(built):
    from infera_amd import capi

    assert capi.device_count() >= 1, capi.get_devices()
    return capi


def run(api, tmp_path, blob, *inputs):
    """one load, one call: the inputs' rows side by side, as a multi-input model takes them"""
    api.load_model("gs", W.write(str(tmp_path / "gs.onnx"), blob))
    try:
        rows = np.ascontiguousarray(np.hstack([np.asarray(a, np.float32).reshape(len(a), -1) for a in inputs]))
        return api.get_plan("gs"), api.predict_from_blob("gs", rows.tobytes()).reshape(len(rows), -1)
    finally:
        api.unload_model("gs")


def check(got, x, grid, mode, padding, align, against64=True):
    want = R.grid_sample32(x, grid, mode, padding, align).reshape(len(x), -1)
    diff = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert not len(diff), (len(diff), int(diff[0]), float(got.flat[diff[0]]), float(want.flat[diff[0]]))
    if against64:
        assert R.tie_distance(grid, x.shape[2:], mode, padding, align).min() >= 2.0 ** -10  # (of the inputs: both precisions pick the same pixels)
        err = float(np.abs(got.astype(np.float64) - R.grid_sample64(x, grid, mode, padding, align).reshape(len(x), -1)).max())
        assert err <= (0.0 if mode == "nearest" else MARGIN * R.bound(x.shape[2:], x)), err


def coordinates(coords, n, align):
    """-> (what the model is given, the [n,Ho,Wo,2] grid that stands for)"""
    if coords == "affine":
        return THETAS[:n], R.affine_grid32(THETAS[:n], OUT_HW, align)
    grid = R.lattice_grid(n, OUT_HW, HW, align)
    if coords == "planar":  # the model adds the identity grid to the flow, one f32 addition: the grid is that sum
        flow = (grid - W.grid_sample_base(OUT_HW)[None]).astype(np.float32)
        return flow.transpose(0, 3, 1, 2), (flow + W.grid_sample_base(OUT_HW)[None]).astype(np.float32)
    return grid, grid


NCHW_CASES = [(co, 3) + cb for co in ("grid", "planar", "affine") for cb in COMBOS] + \
             [(co, c) + cb for c in (1, 4, 5, 8) for co, cb in (("grid", ("bilinear", "border", 0)), ("affine", ("nearest", "reflection", 1)))]


@pytest.mark.parametrize("coords,c,mode,padding,align", NCHW_CASES)
def test_nchw_every_form_is_the_restatement(api, tmp_path, coords, c, mode, padding, align):
    rng = np.random.default_rng(17)
    blob = W.grid_sample_model(coords, c, HW, OUT_HW, mode, padding, align, flow_order="transpose_first" if align else "add_first")
    for n in (3, 5):
        x = rng.uniform(-1, 1, size=(n, c) + HW).astype(np.float32)
        given, grid = coordinates(coords, n, align)
        plan, got = run(api, tmp_path, blob, x, given)
        k = plan["gridsample"][0]
        assert (k["exec"], k["coords"], k["in_layout"], k["out_layout"]) == (f"gridsample_{mode}_nchw", coords, NCHW, NCHW)
        check(got, x, grid, mode, padding, align)


EMBEDDINGS = {"cq": (True, True), "cq_in": (True, False), "cq_out": (False, True)}
CQ_COMBOS = [("bilinear", "zeros", 0), ("bilinear", "reflection", 1), ("nearest", "border", 0), ("bilinear", "border", 1)]


@pytest.mark.parametrize("combo", range(4))
@pytest.mark.parametrize("c", [4, 8])
@pytest.mark.parametrize("emb", list(EMBEDDINGS))
def test_channel_quads_between_two_convolutions(api, tmp_path, emb, c, combo):
    mode, padding, align = CQ_COMBOS[combo]
    coords = "affine" if combo % 2 else "grid"
    given, grid = coordinates(coords, 1, align)
    pre, post = EMBEDDINGS[emb]
    blob = W.grid_sample_model(coords, c, HW, OUT_HW, mode, padding, align, values=given[0], pre=pre, post=post)
    for n in (3, 5):
        x = (np.random.default_rng(19).integers(-256, 257, size=(n, c) + HW) / 256.0).astype(np.float32)
        plan, got = run(api, tmp_path, blob, x)
        k = plan["gridsample"][0]
        assert plan["activation_layout"] == CQ and (k["exec"], k["in_layout"], k["out_layout"]) == (f"gridsample_{mode}_{emb}", CQ if pre else NCHW, CQ if post else NCHW)
        check(got, x, np.repeat(grid, n, axis=0), mode, padding, align)


@pytest.mark.parametrize("mode,padding,align", COMBOS)
def test_edge_values_follow_the_contract(api, tmp_path, mode, padding, align):
    """grid entries of exactly +-1, +-inf, +-1e30 and NaN: bit for bit the restatement; a NaN coordinate gives NaN; +-inf and 1e30 give what the
    padding mode defines -- nothing under zeros, the edge pixel under border"""
    edge = np.array([-1, 1, np.inf, -np.inf, 1e30, -1e30, np.nan, 0.25], np.float32)
    grid = np.resize(np.stack(np.meshgrid(edge, edge), axis=-1).reshape(-1, 2), (3,) + OUT_HW + (2,)).astype(np.float32)
    x = np.random.default_rng(23).uniform(0.5, 1.5, size=(3, 3) + HW).astype(np.float32)
    _, got = run(api, tmp_path, W.grid_sample_model("grid", 3, HW, OUT_HW, mode, padding, align), x, grid)
    check(got, x, grid, mode, padding, align, against64=False)
    got, g = got.reshape(3, 3, -1), grid.reshape(3, -1, 2)
    assert np.isnan(got[np.isnan(g).any(-1)[:, None, :].repeat(3, 1)]).all()
    big = ((np.abs(g) >= 1e30).any(-1) & ~np.isnan(g).any(-1))[:, None, :].repeat(3, 1)
    assert padding != "zeros" or (got[big] == 0).all()
    assert padding != "border" or (got[big] >= 0.5).all()  # (pixels, never the zero of a missing tap)


def test_the_stn_against_float64(api, tmp_path):
    blob, w = W.stn_model(c=1, size=12)
    x = np.random.default_rng(29).uniform(-1, 1, size=(3, 1, 12, 12)).astype(np.float32)
    _, got = run(api, tmp_path, blob, x)
    want = W.stn_reference(w, x)
    assert np.all(np.abs(got - want) <= 1e-4 * np.abs(want) + 1e-6), float(np.abs(got - want).max())  # (the project's parity bar)
