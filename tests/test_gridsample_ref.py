"""The float32 restatement of the grid-sampling contract (tests/gridsample_ref.py) against torch.nn.functional.grid_sample and affine_grid in
float64 on the CPU, for every mode x padding x align_corners, with grid values from -1.5 to 1.5 so that every padding rule fires.  The bound is
MARGIN u (1 + max(H, W)) max|X| (gridsample_ref.bound), MARGIN a small factor over the largest ratio measured
(profiles/gridsample_error_ratios.txt: 3.39).  The grids keep 2^-10 from every tie, where float32 and float64 pick the same pixels: asserted
of the inputs.  The writer's three models are loaded here too, so this file fails where the operator does not load."""
from __future__ import annotations

import numpy as np
import pytest

from infera_amd import onnx_writer as W

import gridsample_ref as R

MARGIN = 8.0
HW, OUT_HW = (5, 7), (6, 11)


@pytest.mark.parametrize("align", R.ALIGNS)
@pytest.mark.parametrize("padding", R.PADDINGS)
@pytest.mark.parametrize("mode", R.MODES)
def test_the_restatement_is_the_operator(mode, padding, align):
    x = np.random.default_rng(11).uniform(-1, 1, size=(3, 3) + HW).astype(np.float32)
    g = R.lattice_grid(3, OUT_HW, HW, align)
    assert g.min() < -1.2 and g.max() > 1.2 and R.tie_distance(g, HW, mode, padding, align).min() >= 2.0 ** -10  # (of the inputs)
    err = float(np.abs(R.grid_sample32(x, g, mode, padding, align).astype(np.float64) - R.grid_sample64(x, g, mode, padding, align)).max())
    print(f"{mode} {padding} align={align}: max error {err:.3e}, ratio {err / R.bound(HW, x):.3f}")
    assert err <= (0.0 if mode == "nearest" else MARGIN * R.bound(HW, x))


@pytest.mark.parametrize("align", R.ALIGNS)
def test_the_affine_grid_is_the_operator(align):
    import torch

    theta = (np.array([1, 0, 0, 0, 1, 0]) + np.random.default_rng(13).uniform(-0.4, 0.4, size=(3, 6))).astype(np.float32)
    want = torch.nn.functional.affine_grid(torch.from_numpy(theta.astype(np.float64).reshape(3, 2, 3)), (3, 3) + OUT_HW, align_corners=bool(align)).numpy()
    assert np.abs(R.affine_grid32(theta, OUT_HW, align) - want).max() <= 8 * 2.0 ** -24 * 2  # five roundings of values below 2 (measured: 3.4 u)


@pytest.mark.parametrize("coords", ["grid", "planar", "affine"])
def test_the_models_load_as_one_step(built, tmp_path, coords):
    from infera_amd import capi

    capi.load_model("gs", W.write(str(tmp_path / "gs.onnx"), W.grid_sample_model(coords)))
    try:
        steps = capi.get_plan("gs")["plan"]["steps"]
    finally:
        capi.unload_model("gs")
    assert [s["coords"] for s in steps if s["kind"] == "GridSample"] == [coords]
