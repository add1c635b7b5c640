"""Times the decoder operators (hip/deconv.hip, hip/resize.hip), device resident: the writer's conv_autoencoder at 3 x 128 x 128, unet_small at
3 x 256 x 256, single ConvTranspose layers 256 -> 128 on 32 x 32 (k4 s2 p1 and k2 s2) and a nearest / linear Resize x2.  Per shape: ms per
pass, the rate, the fraction of the step's own bound -- 2 C M kh kw H W flop per image at the fp32 MFMA peak for a transposed convolution
(the whole plan's flops for a model), the bytes read and written at the HBM rate for Resize --, the same plan with INFERA_CONVT_MFMA=0,
and torch.nn.functional.conv_transpose2d / interpolate on the same GPU in the same process.
usage (GPU box): python tools/deconv_time.py [--quick]      (--quick: 4x fewer rows)"""
import os
import sys
import tempfile
import time

sys.path.insert(0, os.getcwd())
from infera_amd import capi, onnx_writer as W  # noqa: E402

PEAK, HBM = 157.3e12, 6.3e12  # f32 MFMA flop/s and HBM bytes/s, vendor peaks


def run(name, blob, d, rows, cols, out_cols, dev, reps, knob=None):
    if knob is not None:
        os.environ["INFERA_CONVT_MFMA"] = knob
    try:
        capi.load_model(name, W.write(f"{d}/{name}.onnx", blob))
    finally:
        os.environ.pop("INFERA_CONVT_MFMA", None)
    try:
        d_in, d_out = capi.DeviceBuffer(dev, rows * cols * 4), capi.DeviceBuffer(dev, rows * out_cols * 4)
        capi.synth_fill(d_in, 42, 0, rows, cols)
        capi.predict_device(name, d_in, rows, cols, d_out)
        ms = capi.time_predict_device(name, d_in, rows, cols, d_out, reps) / reps
        plan = capi.get_plan(name)
        return ms, plan
    finally:
        capi.unload_model(name)


def torch_ms(fn, reps):
    import torch

    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def main():
    import numpy as np
    import torch
    import torch.nn.functional as F

    quick = "--quick" in sys.argv
    d = tempfile.mkdtemp()
    dev = capi.device_ordinal(0)
    reps = 5
    print(f"peaks: {PEAK / 1e12:.1f} TFLOP/s fp32 MFMA, {HBM / 1e12:.1f} TB/s HBM; torch {torch.__version__}", flush=True)
    # ---- single transposed convolutions: 256 -> 128 on 32 x 32, channel-quad in, NCHW out.  The layer reads channel quads only behind another
    # layer, so the model is an identity 1x1 Conv + the layer; the 1x1 Conv is also timed as a model of its own and subtracted.  That model pays
    # its own launch and its own NCHW store, so the "layer ~" time, its TFLOP/s and its bound fraction are ESTIMATES (the whole-model rows below are not) ----
    rows = 64 if quick else 256
    for label, g in (("convt_256_128_32x32_k4_s2_p1", dict(C=256, M=128, H=32, W=32, k=4, s=2, p=1)), ("convt_256_128_32x32_k2_s2", dict(C=256, M=128, H=32, W=32, k=2, s=2))):
        blob, spec = W.conv_transpose_model(g, pre=False, post=False)
        k = W._pair(g["k"])
        flops = 2.0 * g["C"] * g["M"] * k[0] * k[1] * g["H"] * g["W"]
        cols, oc = int(np.prod(spec["in_shape"])), int(np.prod(spec["out_shape"]))
        # NCHW in and out (the layer alone is a model's first and last layer): the generic kernel
        gms, _ = run(label + "_nchw", blob, d, rows, cols, oc, dev, reps)
        # channel-quad input (an identity 1x1 Conv in front, timed by itself below and subtracted), NCHW out: the MFMA phase kernel
        blob2, _ = W.conv_transpose_model(g, pre=True, post=False)
        ms_on, plan = run(label + "_mfma", blob2, d, rows, cols, oc, dev, reps)
        ms_off, plan_off = run(label + "_generic", blob2, d, rows, cols, oc, dev, reps, knob="0")
        pre_blob = W.model("pre", [W.node("Conv", ["X", "W"], ["Y"], [W.attr_ints("kernel_shape", [1, 1])], name="pre")],
                           [W.tensor("W", np.eye(g["C"], dtype=np.float32)[:, :, None, None])], [W.value_info("X", ["N", g["C"], g["H"], g["W"]])],
                           [W.value_info("Y", ["N", g["C"], g["H"], g["W"]])])
        pre_ms, _ = run(label + "_pre", pre_blob, d, rows, cols, cols, dev, reps)
        x = torch.randn(rows, g["C"], g["H"], g["W"], device="cuda")
        w = torch.randn(g["C"], g["M"], k[0], k[1], device="cuda")
        b = torch.randn(g["M"], device="cuda")
        t_ms = torch_ms(lambda: F.conv_transpose2d(x, w, b, stride=g["s"], padding=g.get("p", 0)), reps)
        bound_ms = rows * flops / PEAK * 1e3
        print(f"{label:<30} rows={rows}: {plan['convt'][0]['kernel']} (+ identity 1x1 Conv {pre_ms:.3f} ms, NCHW-reading generic conv2d) {ms_on:8.3f} ms -> layer ~{ms_on - pre_ms:8.3f} ms (estimate: model minus the 1x1 Conv timed alone)"
              f"  {rows * flops / max(ms_on - pre_ms, 1e-9) / 1e9:8.2f} TFLOP/s  bound fraction {bound_ms / max(ms_on - pre_ms, 1e-9):5.3f}"
              f" | {plan_off['convt'][0]['kernel']} {ms_off:8.3f} ms -> ~{ms_off - pre_ms:8.3f} ms | NCHW in/out generic {gms:8.3f} ms | torch conv_transpose2d {t_ms:8.3f} ms", flush=True)
    # ---- whole models ----
    for label, (blob, spec), rows in (("conv_autoencoder_3x128x128", W.conv_autoencoder((3, 16, 32), 128), 64 if quick else 256),
                                      ("unet_small_3x256x256", W.unet_small(3, 3, 256), 16 if quick else 64)):
        cols = int(np.prod(spec["in_shape"]))
        ms_on, plan = run(label, blob, d, rows, cols, cols, dev, reps)
        ms_off, _ = run(label + "_generic", blob, d, rows, cols, cols, dev, reps, knob="0")
        flops = plan["plan"]["flops_per_row"]
        print(f"{label:<30} rows={rows}: {ms_on:8.3f} ms  {rows / ms_on * 1e3:9.1f} images/s  {rows * flops / ms_on / 1e9:7.2f} TFLOP/s  bound fraction {rows * flops / PEAK * 1e3 / ms_on:5.3f}"
              f" | INFERA_CONVT_MFMA=0 {ms_off:8.3f} ms  x{ms_off / ms_on:5.2f}", flush=True)
    # ---- Resize x2 of 64 x 64 x 64 ----
    rows = 64 if quick else 256
    for mode, tmode in (("nearest", "nearest"), ("linear", "bilinear")):
        blob, spec = W.resize_model(64, (64, 64), scales=(2.0, 2.0), mode=mode, coord="asymmetric" if mode == "nearest" else "half_pixel", nearest_mode="floor")
        cols, oc = int(np.prod(spec["in_shape"])), int(np.prod(spec["out_shape"]))
        ms, _ = run("resize_" + mode, blob, d, rows, cols, oc, dev, reps)
        x = torch.randn(rows, 64, 64, 64, device="cuda")
        t_ms = torch_ms(lambda: F.interpolate(x, scale_factor=2, mode=tmode), reps)
        bound_ms = rows * (cols + oc) * 4 / HBM * 1e3
        print(f"resize2d_{mode}_64x64x64_x2 (NCHW) rows={rows}: {ms:8.3f} ms  {rows * (cols + oc) * 4 / ms / 1e9:7.3f} TB/s  HBM fraction {bound_ms / ms:5.3f} | torch interpolate {t_ms:8.3f} ms", flush=True)


if __name__ == "__main__":
    main()
