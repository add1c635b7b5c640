"""Times the quantised convolution step (hip/qconv.hip) device-resident: the writer's ResNet-18 (width 64, 224 x 224, 1024 images as
bench.py --workload resnet18 takes them) as the float model on the default plan and as its QDQ twin (BatchNormalization folded, global
max pool), then every big layer of it alone as a one-layer QDQ model (NCHW in, channel quads out) with its achieved int8 rate against
the int8 MFMA peak.  REPS timed repetitions of 3 passes after a warm call, medians.
The model files are written to --models DIR once and read from there afterwards, so a checkout of ANOTHER commit can time the same
files: run this file from that checkout's root with --models pointing at the same directory and --no-layers.
usage (GPU box): python tools/quantized_conv_time.py [--models DIR] [--rows N] [--no-layers]"""
import argparse
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.getcwd())
from infera_amd import capi, onnx_writer as W  # noqa: E402

PEAK_I8 = 5.0e15  # dense int8 MFMA rate: twice the ~2.5 PFLOP/s of bf16 (v_mfma_i32_16x16x64_i8: the bf16 form's cycles at twice the K)
REPS = 7
# (C, H = W, M, k, stride, pad) of ResNet-18's convolutions at 224 x 224, and how many of each the net holds
LAYERS = [("stem 7x7/2", 3, 224, 64, 7, 2, 3, 1), ("stage1 3x3", 64, 56, 64, 3, 1, 1, 4), ("stage2 3x3", 128, 28, 128, 3, 1, 1, 3), ("stage3 3x3", 256, 14, 256, 3, 1, 1, 3),
          ("stage4 3x3", 512, 7, 512, 3, 1, 1, 3), ("stage2 3x3/2", 64, 56, 128, 3, 2, 1, 1), ("stage2 1x1/2", 64, 56, 128, 1, 2, 0, 1)]


def timed(dev, name, path, rows, cols, out_per_row, rng):
    capi.load_model(name, path)
    x = rng.uniform(-1, 1, (rows, cols)).astype(np.float32)
    d_in, d_out = capi.DeviceBuffer(dev, x.nbytes), capi.DeviceBuffer(dev, rows * out_per_row * 4)
    d_in.upload(x)
    del x
    capi.predict_device(name, d_in, rows, cols, d_out)
    ms = sorted(capi.time_predict_device(name, d_in, rows, cols, d_out, 3) / 3 for _ in range(REPS))
    plan = capi.get_plan(name)
    capi.unload_model(name)
    del d_in, d_out
    return ms[len(ms) // 2], ms[0], ms[-1], plan


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default=os.path.join(tempfile.gettempdir(), "infera_qconv_models"))
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--no-layers", action="store_true")
    a = ap.parse_args()
    os.makedirs(a.models, exist_ok=True)
    f32_path, qdq_path = os.path.join(a.models, "resnet18_f32.onnx"), os.path.join(a.models, "resnet18_qdq.onnx")
    if not os.path.exists(f32_path):
        W.write(f32_path, W.resnet18())
    if not os.path.exists(qdq_path):
        W.write(qdq_path, W.quantized_conv_from_spec(W.quantized_conv_spec("resnet18", (3, 224, 224), width=64, classes=1000, calib_rows=1)))
    dev = capi.device_ordinal(0)
    rng = np.random.default_rng(1)
    cols = 3 * 224 * 224
    res = {}
    for tag, path in (("float", f32_path), ("qdq", qdq_path)):
        med, lo, hi, plan = timed(dev, "r18_" + tag, path, a.rows, cols, 1000, rng)
        kinds = [s["kind"] for s in plan["plan"]["steps"]]
        res[tag] = med
        print(f"resnet18 {tag:<6} {a.rows} images: median {med:9.3f} ms (min {lo:9.3f}, max {hi:9.3f}, n={REPS}) = {a.rows / med * 1e3:9.1f} images/s; layout "
              f"{plan['activation_layout']}; steps: {kinds.count('Conv2d')} Conv2d, {kinds.count('QConv2d')} QConv2d, {kinds.count('FakeQuant')} FakeQuant", flush=True)
    print(f"resnet18 qdq / float = {res['qdq'] / res['float']:.3f}", flush=True)
    if a.no_layers:
        return
    for what, C, hw, M, k, s, p, count in LAYERS:
        spec = W.quantized_conv_spec("layer", (C, hw, hw), m=M, k=k, stride=s, pads=p, act="Relu", pooled=True, calib_rows=1)
        path = W.write(os.path.join(a.models, "layer.onnx"), W.quantized_conv_from_spec(spec))
        rows = max(16, min(a.rows, (1 << 28) // (C * hw * hw)))
        med, lo, hi, plan = timed(dev, "layer", path, rows, C * hw * hw, M, rng)
        ops = plan["plan"]["flops_per_row"] * rows
        q = plan["qconv"][0]
        print(f"layer {what:<13} C{C:<3} {hw:>3}x{hw:<3} -> M{M:<3} (x{count} in the net) {rows:>5} images: median {med:8.3f} ms (min {lo:8.3f}, max {hi:8.3f}) = "
              f"{ops / med / 1e9:8.2f} Top/s = {ops / med * 1e3 / PEAK_I8:6.4f} of the int8 MFMA peak; window in {q['input_window']}, {q['in_layout']} -> {q['out_layout']}", flush=True)


if __name__ == "__main__":
    main()
