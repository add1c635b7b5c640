"""Times the SpatialNorm kernels (hip/spatialnorm.hip), device resident: GroupNorm(32) + SiLU on 64 x 32 x 32 (the fused kernel) and on
256 x 64 x 64 (E = 32,768: the general plan), InstanceNorm on 128 x 64 x 64.  Per shape, on an NCHW tensor (the layer is the whole model) and on
channel-quad planes (identity 1x1 layers around it; the same model without the layer is timed and subtracted, so those rows are ESTIMATES):
ms per pass, rows/s, bytes/s counted as 8 bytes per element (one read, one write), the fraction of the read+write stream ceiling, the same
model with INFERA_SPATIALNORM_FUSED=0, and torch.nn.functional.group_norm (+ silu) on the same GPU in the same process.
usage (GPU box): python tools/spatialnorm_time.py [--quick]      (--quick: 4x fewer rows)"""
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.getcwd())
from infera_amd import capi, onnx_writer as W  # noqa: E402

STREAM_RW, STREAM_R = (5.2e12, 5.6e12), (6.1e12, 6.3e12)  # measured read+write and pure-read stream ceilings, bytes/s


def run(name, blob, d, rows, cols, dev, reps, knob=None):
    if knob is not None:
        os.environ["INFERA_SPATIALNORM_FUSED"] = knob
    try:
        capi.load_model(name, W.write(f"{d}/{name}.onnx", blob))
    finally:
        os.environ.pop("INFERA_SPATIALNORM_FUSED", None)
    try:
        d_in, d_out = capi.DeviceBuffer(dev, rows * cols * 4), capi.DeviceBuffer(dev, rows * cols * 4)
        capi.synth_fill(d_in, 42, 0, rows, cols)
        capi.predict_device(name, d_in, rows, cols, d_out)
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


def identity_pair(c, hw):
    """the identity 1x1 Conv + identity 1x1 ConvTranspose that surround the layer in the channel-quad models, alone"""
    net = W._DecoderNet(0)
    eye = np.eye(c, dtype=np.float32)[:, :, None, None]
    cur = net.convt(net.conv("X", c, c, 1, 1, 0, bias=False, w=eye), c, c, 1, 1, 0, bias=False, w=eye)
    return net.finish("pair", W.value_info("X", ["N", c] + list(hw)), cur, ["N", c] + list(hw))[0]


def main():
    import torch
    import torch.nn.functional as F

    quick = "--quick" in sys.argv
    d = tempfile.mkdtemp()
    dev = capi.device_ordinal(0)
    reps = 20
    print(f"stream ceilings: read+write {STREAM_RW[0] / 1e12:.1f}-{STREAM_RW[1] / 1e12:.1f} TB/s, pure read {STREAM_R[0] / 1e12:.1f}-{STREAM_R[1] / 1e12:.1f} TB/s; "
          f"bytes/s below = 8 bytes per element over the time; torch {torch.__version__}", flush=True)
    shapes = [("groupnorm32_silu_64x32x32", 64, 32, (32, 32), "GroupNormalization", "Silu", 4096),
              ("groupnorm32_silu_256x64x64", 256, 32, (64, 64), "GroupNormalization", "Silu", 256),
              ("instancenorm_128x64x64", 128, 128, (64, 64), "InstanceNormalization", None, 512)]
    for label, c, g, hw, op, act, rows in shapes:
        rows = rows // 4 if quick else rows
        cols = c * hw[0] * hw[1]
        byts = 8.0 * rows * cols
        pair_ms, _ = run(label + "_pair", identity_pair(c, hw), d, rows, cols, dev, reps)
        for layout, embed in (("NCHW", {}), ("NC/4HW4", dict(pre=True, post=True))):
            blob, _ = W.spatial_norm_model(c, g, hw, op=op, form="op21", act=act, **embed)
            for knob in (None, "0"):
                ms, plan = run(label, blob, d, rows, cols, dev, reps, knob)
                kernels = "+".join(k["kernel"] for k in plan["spatialnorm"])
                assert all(k["in_layout"] == layout for k in plan["spatialnorm"]), plan["spatialnorm"]
                own = ms - pair_ms if embed else ms
                est = "~" if embed else " "
                print(f"{label:<28} {layout:<8} {'default' if knob is None else 'FUSED=0':<8} {kernels:<36} rows={rows:>5} model {ms:8.3f} ms  layer{est}{own:8.3f} ms  "
                      f"{rows / own * 1e3:10.0f} rows/s  {byts / own / 1e6:8.1f} GB/s  = {byts / own * 1e3 / STREAM_RW[1]:5.3f}-{byts / own * 1e3 / STREAM_RW[0]:5.3f} of read+write stream"
                      + (f"  (identity pair alone {pair_ms:.3f} ms)" if embed else ""), flush=True)
        x = torch.randn(rows, c, *hw, device="cuda")
        w, b = torch.randn(c, device="cuda"), torch.randn(c, device="cuda")
        fn = (lambda: F.silu(F.group_norm(x, g, w, b, 1e-5))) if act else (lambda: F.group_norm(x, g, w, b, 1e-5))
        t = torch_ms(fn, reps)
        print(f"{label:<28} torch    F.group_norm{' + F.silu' if act else '':<10} rows={rows:>5} {t:8.3f} ms  {rows / t * 1e3:10.0f} rows/s  {byts / t / 1e6:8.1f} GB/s (same byte count)", flush=True)
        x = None


if __name__ == "__main__":
    main()
