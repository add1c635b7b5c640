"""Times the ChannelNorm kernel (hip/channelnorm.hip), device resident, on the ConvNeXt-T stage shapes 96 x 56 x 56, 192 x 28 x 28, 384 x 14 x 14
and 768 x 7 x 7.  The step reads a tensor a step wrote, so it is never the whole model: on an NCHW tensor it stands behind a Relu, on
channel-quad planes between an identity 1x1 Conv and an identity 1x1 ConvTranspose; the same model without the step is timed on the same
buffers in the same run and subtracted, so the step's rows are ESTIMATES.  Per shape and layout: the step's ms per pass with the register
form and with INFERA_CHANNELNORM_REGS=0 (the re-read form), its bytes/s counted as 8 bytes per element (one read, one write), and beside it
the plain pass over the same bytes on the same buffers (the Relu alone: one read and one write per element, a copy kernel).  Then
torch.nn.functional.layer_norm over the permuted tensor on 16 CPU threads, and a ConvNeXt-T topology's images/s through predict_device.
Medians of 5 windows of 20 passes.
usage (GPU box): python tools/channelnorm_time.py [--quick]      (--quick: 4x fewer rows, no whole model)"""
import os
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.getcwd())
from infera_amd import capi, onnx_writer as W  # noqa: E402

REPS, WINDOWS = 20, 5


def timed(name, blob, d, rows, cols, out_cols, dev, knob=None):
    """median ms per pass of the model `blob`, and its plan"""
    if knob is not None:
        os.environ["INFERA_CHANNELNORM_REGS"] = knob
    try:
        capi.load_model(name, W.write(f"{d}/{name}.onnx", blob))
    finally:
        os.environ.pop("INFERA_CHANNELNORM_REGS", None)
    try:
        d_in, d_out = capi.DeviceBuffer(dev, rows * cols * 4), capi.DeviceBuffer(dev, rows * out_cols * 4)
        capi.synth_fill(d_in, 42, 0, rows, cols)
        capi.predict_device(name, d_in, rows, cols, d_out)
        ms = statistics.median(capi.time_predict_device(name, d_in, rows, cols, d_out, REPS) / REPS for _ in range(WINDOWS))
        return ms, capi.get_plan(name)
    finally:
        capi.unload_model(name)


def without_step(c, hw, front):
    """channel_norm_model's surroundings alone: the Relu, or the identity 1x1 Conv + ConvTranspose"""
    net = W._ConvNextNet()
    eye = np.eye(c, dtype=np.float32).reshape(c, c, 1, 1)
    if front == "relu":
        cur = net.op("Relu", ["X"], "front")
    else:
        cur = net.op("Conv", ["X", net.f("front_w", eye)], "front", [W.attr_ints("kernel_shape", [1, 1])])
        cur = net.op("ConvTranspose", [cur, net.f("back_w", eye)], "back", [W.attr_ints("strides", [1, 1]), W.attr_ints("pads", [0, 0, 0, 0])])
    return W.model("without", net.nodes, net.inits, [W.value_info("X", ["N", c] + list(hw))], [W.value_info(cur, ["N", c] + list(hw))], opset=20)


def main():
    import torch
    import torch.nn.functional as F

    quick = "--quick" in sys.argv
    d = tempfile.mkdtemp()
    dev = capi.device_ordinal(0)
    print(f"bytes/s below = 8 bytes per element over the time; step = model - the same model without the step (an estimate); torch {torch.__version__}", flush=True)
    for c, hw, rows in ((96, (56, 56), 256), (192, (28, 28), 512), (384, (14, 14), 1024), (768, (7, 7), 2048)):
        rows = rows // 4 if quick else rows
        cols = c * hw[0] * hw[1]
        byts = 8.0 * rows * cols
        label = f"{c}x{hw[0]}x{hw[1]}"
        relu_ms, _ = timed("relu", without_step(c, hw, "relu"), d, rows, cols, cols, dev)
        pair_ms, _ = timed("pair", without_step(c, hw, "conv"), d, rows, cols, cols, dev)
        print(f"{label:<12} plain pass (Relu alone, the same buffers) rows={rows:>5} {relu_ms:8.3f} ms  {byts / relu_ms / 1e6:8.1f} GB/s", flush=True)
        for layout, front, base in (("NCHW", "relu", relu_ms), ("NC/4HW4", "conv", pair_ms)):
            blob, _ = W.channel_norm_model(c, hw, spelling="layernorm2d", front=front)
            for knob in (None, "0"):
                ms, plan = timed("cn", blob, d, rows, cols, cols, dev, knob)
                (k,) = plan["channelnorm"]
                assert k["in_layout"] == layout, plan["channelnorm"]
                own = ms - base
                print(f"{label:<12} {layout:<8} {k['kernel']:<19} rows={rows:>5} model {ms:8.3f} ms  without the step {base:8.3f} ms  step~{own:8.3f} ms  "
                      f"{byts / own / 1e6:8.1f} GB/s  = {relu_ms / own:5.3f} of the plain pass's rate", flush=True)
        torch.set_num_threads(16)
        n_cpu = max(1, rows // 16)
        x = torch.randn(n_cpu, c, *hw)
        w, b = torch.randn(c), torch.randn(c)
        fn = lambda: F.layer_norm(x.permute(0, 2, 3, 1), (c,), w, b, 1e-6).permute(0, 3, 1, 2).contiguous()  # noqa: E731
        fn()
        t0 = time.perf_counter()
        for _ in range(3):
            fn()
        t = (time.perf_counter() - t0) / 3 * 1e3
        print(f"{label:<12} torch, 16 CPU threads, F.layer_norm over the permuted tensor rows={n_cpu:>5} {t:8.3f} ms  {8.0 * n_cpu * cols / t / 1e6:8.1f} GB/s (same byte count)", flush=True)
    if quick:
        return
    spec = W.convnext_spec(img=(3, 224, 224), widths=(96, 192, 384, 768), depths=(3, 3, 9, 3), classes=1000, weight_scale=0.5)
    rows, cols = 64, 3 * 224 * 224
    for style in ("torchvision", "hf"):
        ms, plan = timed("convnext_t", W.convnext_from_spec(spec, style=style), d, rows, cols, 1000, dev)
        kinds = [s["kind"] for s in plan["plan"]["steps"]]
        forms = sorted({k["kernel"] for k in plan["channelnorm"]})
        print(f"ConvNeXt-T topology ({style} spelling) rows={rows} {ms:8.3f} ms  {rows / ms * 1e3:8.1f} img/s  layout {plan['activation_layout']}  "
              f"{kinds.count('ChannelNorm')} ChannelNorm steps ({', '.join(forms)}), {kinds.count('Conv2d')} Conv2d, {kinds.count('Unary')} Unary (Gelu)", flush=True)


if __name__ == "__main__":
    main()
