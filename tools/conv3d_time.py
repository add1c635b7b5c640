"""Times the 3-D convolution kernels (hip/conv3d.hip), device resident: R3D-18's distinct layers alone at the sizes a 3 x 16 x 112 x 112 clip
gives them -- the stem 3 -> 64 (3,7,7)/(1,2,2) and the 3x3x3 layers at 64, 128, 256 and 512 channels -- and the whole R3D-18 topology
(onnx_writer.r3d_net).  Per shape: ms per pass on conv3d_mfma, the rate and its fraction of the fp32 MFMA peak (2 K M OD OH OW flop per clip
over the time of the whole call: an end-to-end figure, not a kernel's), the same plan with INFERA_CONV3D_STAGE=1 (the input window through
LDS where it fits) and with INFERA_CONV3D_MFMA=0 (conv3d_generic), and torch float32 F.conv3d / the eager model on the same weights on the same GPU in
the same process.
usage (GPU box): python tools/conv3d_time.py [--quick]      (--quick: one clip per pass instead of four)"""
import os
import sys
import tempfile
import time

sys.path.insert(0, os.getcwd())
from infera_amd import capi, onnx_writer as W  # noqa: E402

PEAK = 157.3e12  # f32 MFMA flop/s, vendor peak
KNOBS = ("INFERA_CONV3D_STAGE", "INFERA_CONV3D_MFMA")


def run(name, blob, d, rows, cols, out_cols, dev, reps, knob=None):
    if knob is not None:
        os.environ[knob[0]] = knob[1]
    try:
        capi.load_model(name, W.write(f"{d}/{name}.onnx", blob))
    finally:
        for k in KNOBS:
            os.environ.pop(k, None)
    try:
        d_in, d_out = capi.DeviceBuffer(dev, rows * cols * 4), capi.DeviceBuffer(dev, rows * out_cols * 4)
        capi.synth_fill(d_in, 42, 0, rows, cols)
        capi.predict_device(name, d_in, rows, cols, d_out)  # (warm-up: code objects, scratch)
        ms = capi.time_predict_device(name, d_in, rows, cols, d_out, reps) / reps
        return ms, capi.get_plan(name)
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

    rows = 1 if "--quick" in sys.argv else 4
    d = tempfile.mkdtemp()
    dev = capi.device_ordinal(0)
    reps = 30
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    print(f"peak: {PEAK / 1e12:.1f} TFLOP/s fp32 MFMA; torch {torch.__version__}; {rows} clips per pass, {reps} passes per figure", flush=True)
    ws = W._WeightStream(5)
    layers = [("stem_3_64_k377_s122", 3, 64, (16, 112, 112), (3, 7, 7), (1, 2, 2), (1, 3, 3)), ("conv_64_64_k3_16x56x56", 64, 64, (16, 56, 56), (3, 3, 3), (1, 1, 1), (1, 1, 1)),
              ("conv_128_128_k3_8x28x28", 128, 128, (8, 28, 28), (3, 3, 3), (1, 1, 1), (1, 1, 1)), ("conv_256_256_k3_4x14x14", 256, 256, (4, 14, 14), (3, 3, 3), (1, 1, 1), (1, 1, 1)),
              ("conv_512_512_k3_2x7x7", 512, 512, (2, 7, 7), (3, 3, 3), (1, 1, 1), (1, 1, 1))]
    for label, c, m, dhw, k, st, pad in layers:
        w, b = ws.take((m, c, *k), c * int(np.prod(k))), ws.take((m,), c)
        blob = W.conv3d_layer(w, b, dhw, act="Relu", strides=list(st), pads=list(pad) * 2)
        out = [(dhw[i] + 2 * pad[i] - k[i]) // st[i] + 1 for i in range(3)]
        cols, oc = c * int(np.prod(dhw)), m * int(np.prod(out))
        ms, plan = run(label, blob, d, rows, cols, oc, dev, reps)
        step = plan["plan"]["steps"][0]
        flops = plan["plan"]["flops_per_row"]
        ms_staged, plan_s = run(label + "_staged", blob, d, rows, cols, oc, dev, reps, knob=("INFERA_CONV3D_STAGE", "1"))
        staged = plan_s["plan"]["steps"][0]
        ms_generic, _ = run(label + "_generic", blob, d, rows, cols, oc, dev, max(2, reps // 3), knob=("INFERA_CONV3D_MFMA", "0"))
        x, wt, bt = torch.randn(rows, c, *dhw, device="cuda"), torch.tensor(w, device="cuda"), torch.tensor(b, device="cuda")
        t_ms = torch_ms(lambda: F.relu(F.conv3d(x, wt, bt, stride=st, padding=pad)), reps)
        print(f"{label:<26} {step['exec']} window={step['input_window']}: {ms:8.3f} ms  {rows * flops / ms / 1e9:7.2f} TFLOP/s  peak fraction "
              f"{rows * flops / PEAK * 1e3 / ms:5.3f} | INFERA_CONV3D_STAGE=1 window={staged['input_window']} lds={staged['lds_bytes']:>6} {ms_staged:8.3f} ms | conv3d_generic {ms_generic:8.3f} ms  x{ms_generic / ms:5.2f} | torch F.conv3d+relu "
              f"{t_ms:8.3f} ms  x{t_ms / ms:5.2f}", flush=True)
    # ---- the whole R3D-18 topology on 3 x 16 x 112 x 112 clips ----
    blob, ops = W.r3d_net(widths=(64, 128, 256, 512), blocks=2, in_dhw=(16, 112, 112), classes=400, stem_k=(3, 7, 7), pool=False)
    cols = 3 * 16 * 112 * 112
    ms, plan = run("r3d18", blob, d, rows, cols, 400, dev, reps)
    flops = plan["plan"]["flops_per_row"]
    ms_staged, _ = run("r3d18_staged", blob, d, rows, cols, 400, dev, reps, knob=("INFERA_CONV3D_STAGE", "1"))
    ms_generic, _ = run("r3d18_generic", blob, d, rows, cols, 400, dev, 2, knob=("INFERA_CONV3D_MFMA", "0"))
    T = lambda a: torch.tensor(np.asarray(a), device="cuda")  # noqa: E731
    tops = [tuple(T(a) if isinstance(a, np.ndarray) else [T(e) for e in a] if isinstance(a, list) and isinstance(a[0], np.ndarray) else a for a in o) for o in ops]
    x = torch.randn(rows, 3, 16, 112, 112, device="cuda")

    def eager():
        v = [x]
        for o in tops:
            if o[0] == "conv":
                _, w, (sc, b, mu, var), st, pad, relu, src = o
                y = F.batch_norm(F.conv3d(v[src], w, stride=st, padding=pad), mu, var, sc, b, False, 0.0, 1e-5)
                v.append(F.relu(y) if relu else y)
            elif o[0] == "add":
                v.append(F.relu(v[o[1]] + v[o[2]]))
            else:
                return v[-1].mean(dim=(2, 3, 4)) @ o[1] + o[2]

    with torch.no_grad():
        t_ms = torch_ms(eager, reps)
    print(f"r3d18_3x16x112x112 ({flops / 1e9:.1f} GFLOP per clip): {ms:8.3f} ms  {rows / ms * 1e3:7.1f} clips/s  {rows * flops / ms / 1e9:7.2f} TFLOP/s  peak fraction "
          f"{rows * flops / PEAK * 1e3 / ms:5.3f} | INFERA_CONV3D_STAGE=1 {ms_staged:8.3f} ms | conv3d_generic {ms_generic:8.3f} ms  x{ms_generic / ms:5.2f} | torch eager (BatchNormalization unfolded) {t_ms:8.3f} ms  x{t_ms / ms:5.2f}", flush=True)


if __name__ == "__main__":
    main()
