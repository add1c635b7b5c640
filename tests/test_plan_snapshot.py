"""One small model per step family, and two things about each.  Without a GPU: the plan infera_load_model makes for it (steps, fusion
decisions, activation layout, scratch, narrow edges, everything infera_hip_get_plan reports but the devices of the box) equals the JSON
recorded under tests/golden/plans/ -- exactly; a change of the load-time code that is meant to leave plans alone shows here first.
INFERA_PLAN_SNAPSHOT_WRITE=1 records the fixtures instead of comparing.  On a GPU: a model that is loaded, run, unloaded and loaded again
gives the same bits -- every device table of every family is uploaded, handed to its kernel and freed through DeviceModel's one list.

None of the models has a run of small Dense layers: those are given a load-time compiled kernel only where a GPU is visible, so their plans
differ between boxes."""
from __future__ import annotations

import json
import os

import numpy as np
import pytest

from infera_amd import onnx_writer as W
from tests.test_conv_split_plan import shortcut_block

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plans")

# (each one a model a CPU test of its family already loads: test_quantized, test_half, test_quantized_conv, test_conv_split_plan, test_prep,
# test_recurrent, test_transformer, test_nearest)
MODELS = {
    "qdense_chain": lambda: W.quantized_from_spec(W.quantized_mlp_spec((128, 256, 64, 1))),  # the two middle edges carry bytes
    "hdense_chain": lambda: W.half_from_spec(W.half_mlp_spec((128, 256, 64, 1))),            # ... halves
    "qconv": lambda: W.quantized_conv_from_spec(W.quantized_conv_spec("layer", (8, 9, 9), m=8, k=3, pads=1, act="Relu")),
    "qconv_resnet": lambda: W.quantized_conv_from_spec(W.quantized_conv_spec("resnet", (3, 32, 32), width=8, seed=77)),
    "shortcut_block": lambda: shortcut_block(False),  # patch stem, split convolutions, a fused residual Add, a folded 1x1 shortcut, a tiled head
    "resnet_stem": lambda: W.resnet18(classes=10, in_hw=32, width=64),  # ... and the split stem with its fused MaxPool
    "tree_ensemble": lambda: W.tree_ensemble(kind="classifier", trees=8, depth=4, output="probabilities", seed=4),
    "svm_probabilities": lambda: W.svm(n_sv=64, probabilities=True, output="probabilities", seed=6),
    "prep": lambda: W.prep_from_spec(W.prep_spec()),
    "lstm": lambda: W.recurrent_from_spec(W.recurrent_spec("LSTM", T=6, F=4, H=8, initial=0.5)),
    "encoder": lambda: W.transformer_from_spec(W.transformer_spec(T=24, F=8, E=64, h=4, ff=256, layers=1, causal=True)),
    "kmeans": lambda: W.kmeans_from_spec(W.kmeans_spec(30, 100, seed=3), "gemm", "label"),
}

# The plan alone, for the families the reload test's random rows cannot feed (indices, masks) or need not: again each one a model a CPU test
# of its family already loads (test_deconv, test_spatial_norm, test_vit, test_channel_norm, test_embed, test_nearest,
# test_recurrent, test_onnx_ml_domain, test_onnx_breadth, test_half).  The writers that also return what they drew give (bytes, ...).
# (No padded text encoder: its small feed-forward layers are a load-time compiled chain where a GPU is visible, see above.)
PLAN_ONLY = {
    "conv_autoencoder": lambda: W.conv_autoencoder()[0],
    "upsample_decoder": lambda: W.upsample_decoder()[0],
    "unet_group": lambda: W.unet_small(norm="group")[0],
    "style_net": lambda: W.style_net_small()[0],
    "vit": lambda: W.vit_from_spec(W.vit_spec()),
    "convnext": lambda: W.convnext_from_spec(W.convnext_spec()),
    "embedding": lambda: W.embedding_from_spec(W.embedding_spec(), tail="none"),  # (the mlp tail is a run of small Dense layers)
    "knn_search": lambda: W.knn_search_from_spec(W.kmeans_spec(30, 100, seed=3), k=5),  # CDist
    "gru_time_major": lambda: W.recurrent_from_spec(W.recurrent_spec("GRU", T=6, F=4, H=8), form="time_major"),
    "sklearn_pipeline": lambda: W.sklearn_pipeline(),
    "mobilenet_v2": lambda: W.mobilenet_v2(),
    "se_net": lambda: W.se_net(),
    "zoo_ops_net": lambda: W.zoo_ops_net()[0],
    "reduce_zoo": lambda: W.reduce_zoo()[0],
    "half_cnn": lambda: W.half_cnn_from_spec(W.half_cnn_spec()),
    "unary_zoo": lambda: W.unary_zoo(),
}


@pytest.fixture(scope="module")
def api(built):
    from infera_amd import capi

    return capi


def _write(tmp_path, family):
    return W.write(str(tmp_path / f"{family}.onnx"), (MODELS.get(family) or PLAN_ONLY[family])())


@pytest.mark.parametrize("family", list(MODELS) + list(PLAN_ONLY))
def test_plan_equals_the_recorded_one(api, tmp_path, family):
    name = "snapshot_" + family
    api.load_model(name, _write(tmp_path, family))
    try:
        plan = api.get_plan(name)
    finally:
        api.unload_model(name)
    for key in ("devices", "device_error"):  # (the box, not the plan)
        plan.pop(key, None)
    fixture = os.path.join(GOLDEN, family + ".json")
    if os.environ.get("INFERA_PLAN_SNAPSHOT_WRITE") == "1":
        os.makedirs(GOLDEN, exist_ok=True)
        with open(fixture, "w") as fh:
            json.dump(plan, fh, indent=1, sort_keys=True)
            fh.write("\n")
    with open(fixture) as fh:
        assert plan == json.load(fh)


@pytest.mark.gpu
@pytest.mark.parametrize("family", list(MODELS))
def test_reloaded_model_gives_the_same_bits(api, tmp_path, family):
    """257 rows: one full 256-row tile and a one-row tail, the smallest count that reaches both."""
    assert api.device_count() >= 1, api.get_devices()
    name, path = "reload_" + family, _write(tmp_path, family)
    api.load_model(name, path)
    try:
        shape = api.get_model_info(name)["input_shape"]
        # (one decimal: integral values among them, which the preprocessing model's category columns match)
        x = np.round(np.random.default_rng(7).normal(0.0, 2.0, (257, int(np.prod(shape[1:])))), 1).astype(np.float32)
        # (images go through the entry that takes tensors of any rank)
        predict = (lambda: api.predict(name, x)) if len(shape) == 2 else (lambda: api.predict_from_blob(name, x.tobytes()))
        first = predict()
    finally:
        api.unload_model(name)
    api.load_model(name, path)
    try:
        second = predict()
    finally:
        api.unload_model(name)
    assert first.size and np.array_equal(first, second) and np.array_equal(first.view(np.uint32), second.view(np.uint32))
