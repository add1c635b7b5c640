"""Times the DeformConv kernels (hip/deformconv.hip), device resident, on two DCN backbone shapes (256 -> 256, 3x3, modulated, at 50 x 68 and
100 x 136, batch 8) and one alignment shape (64 -> 64, 3x3, offset_group = 8, at 180 x 320, batch 2).  Four plans read the SAME device rows -- the
columns X | offsets | mask of onnx_writer.deform_conv_layer -- loaded side by side in one process and timed in turns:
  deformconv_mfma     the layer (SliceCols of its operands + the step)
  conv2d              the ordinary Conv of the same geometry and weights on the X columns: what zero offsets would compute.  A single layer whose
                      result is served keeps its plan in NCHW, so this is the library's NCHW Conv2d kernel, not the channel-quad tiled one
  offset_pass         an elementwise pass (Relu) over the offset columns: the memory floor of reading the offsets once
  deformconv_generic  the layer under INFERA_DEFORMCONV_MFMA=0 (fewer passes: it repeats every sample per output channel)
Every figure is the median over the turns of the time of a whole call (ms), a host clock around work that ends in a device synchronise; the rate
is 2 K M OH OW flop per image over that time: an end-to-end figure, not a kernel's.
usage (GPU box): python tools/deformconv_time.py [--quick]      (--quick: the first shape only)"""
import os
import statistics
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.getcwd())
from infera_amd import capi, onnx_writer as W  # noqa: E402

SHAPES = [("dcn_256_256_k3_50x68", 256, 256, (50, 68), 1, True, 8), ("dcn_256_256_k3_100x136", 256, 256, (100, 136), 1, True, 8),
          ("align_64_64_k3_og8_180x320", 64, 64, (180, 320), 8, False, 2)]
TURNS, REPS = 5, 4


def side_model(kind, w, b, hw, cols, attrs):
    """conv2d / offset_pass over the same three (two) input columns as the layer"""
    c, (h, wd) = w.shape[1], hw
    ins = [W.value_info(nm, ["N", k]) for nm, k in cols]
    if kind == "conv2d":
        nodes = [W.node("Reshape", ["X", "x_shape"], ["x"], name="x_reshape"), W.node("Conv", ["x", "w", "b"], ["Y"], W._attrs3d(attrs), name="conv")]
        inits = [W.tensor("x_shape", np.array([-1, c, h, wd], np.int64)), W.tensor("w", w), W.tensor("b", b)]
        return W.model("conv2d", nodes, inits, ins, [W.value_info("Y", ["N", w.shape[0], h, wd])], opset=19)
    return W.model("offset_pass", [W.node("Relu", ["O"], ["Y"], name="pass")], [], ins, [W.value_info("Y", ["N", cols[1][1]])], opset=19)


def main():
    d = tempfile.mkdtemp()
    dev = capi.device_ordinal(0)
    ws = W._WeightStream(7)
    print(f"{TURNS} turns of {REPS} passes per figure (deformconv_generic: 2 passes); times are whole calls", flush=True)
    for label, c, m, hw, og, mask, rows in SHAPES[:1] if "--quick" in sys.argv else SHAPES:
        w, b = ws.take((m, c, 3, 3), c * 9), ws.take((m,), c)
        attrs = dict(pads=[1, 1, 1, 1], kernel_shape=[3, 3])
        p = hw[0] * hw[1]
        cols = [("X", c * p), ("O", og * 18 * p)] + ([("M", og * 9 * p)] if mask else [])
        in_cols, out_cols = sum(k for _, k in cols), m * p
        blobs = {"deformconv_mfma": W.deform_conv_layer(w, b, hw, mask=mask, offset_group=og, **attrs), "conv2d": side_model("conv2d", w, b, hw, cols, attrs),
                 "offset_pass": side_model("offset_pass", w, b, hw, cols, attrs)}
        d_in = capi.DeviceBuffer(dev, rows * in_cols * 4)
        capi.synth_fill(d_in, 42, 0, rows, in_cols)
        outs, execs, ms = {}, {}, {k: [] for k in blobs}
        for k, blob in blobs.items():
            capi.load_model(k, W.write(f"{d}/{label}_{k}.onnx", blob))
            outs[k] = capi.DeviceBuffer(dev, rows * (cols[1][1] if k == "offset_pass" else out_cols) * 4)
            capi.predict_device(k, d_in, rows, in_cols, outs[k])  # (warm-up: code objects, scratch)
            execs[k] = capi.get_plan(k)
        for _ in range(TURNS):
            for k in blobs:
                ms[k].append(capi.time_predict_device(k, d_in, rows, in_cols, outs[k], REPS) / REPS)
        for k in blobs:
            capi.unload_model(k)
        os.environ["INFERA_DEFORMCONV_MFMA"] = "0"
        try:
            capi.load_model("generic", W.write(f"{d}/{label}_generic.onnx", blobs["deformconv_mfma"]))
        finally:
            os.environ.pop("INFERA_DEFORMCONV_MFMA")
        capi.predict_device("generic", d_in, rows, in_cols, outs["deformconv_mfma"])
        g_ms = capi.time_predict_device("generic", d_in, rows, in_cols, outs["deformconv_mfma"], 2) / 2
        assert capi.get_plan("generic")["deformconv"][0]["exec"] == "deformconv_generic"
        capi.unload_model("generic")
        med = {k: statistics.median(v) for k, v in ms.items()}
        dc = execs["deformconv_mfma"]["deformconv"][0]
        flops = execs["deformconv_mfma"]["plan"]["flops_per_row"] * rows
        t = med["deformconv_mfma"]
        print(f"{label:<28} batch {rows}  {dc['exec']} lds={dc['lds_bytes']}: {t:8.3f} ms (min {min(ms['deformconv_mfma']):.3f} max {max(ms['deformconv_mfma']):.3f})  "
              f"{flops / t / 1e9:6.2f} TFLOP/s | conv2d [{execs['conv2d']['exec'][-1]}] {med['conv2d']:8.3f} ms  deform/conv x{t / med['conv2d']:5.2f} | offset_pass {med['offset_pass']:7.3f} ms  "
              f"deform/pass x{t / med['offset_pass']:6.1f} | deformconv_generic {g_ms:9.3f} ms  generic/mfma x{g_ms / t:6.1f}", flush=True)


if __name__ == "__main__":
    main()
