"""Times the GridSample step (hip/gridsample.hip) device-resident at C = 64 channels, 128 x 128 sampled to 128 x 128 (4 MiB per image on each
side), ROWS images a call, bilinear / zeros / align_corners = 0, under a smooth warp (the identity grid plus a small rotation).
  (1) NCHW to NCHW: the two-input model of the writer -- SliceCols of the image, SliceCols of the grid, GridSample -- and the same model's two
      slices alone read off a plain elementwise pass of this project (Relu) over a buffer of the image's size in the same process: the step's
      own time is the model's minus about one such pass (the slices copy the image and the grid once);
  (2) the affine form on channel quads between an identity Conv 1x1 and an identity ConvTranspose 1x1, minus the two identity layers alone
      (the localisation net of the model is a zero-weight 1x1 Conv to four channels, a pool and a 4 x 6 Gemm);
  (3) torch-ROCm's F.grid_sample on resident float32 tensors of the same shapes, in a process of its own.
REPS timed windows of CALLS calls after a warm call, medians; each leg is a child process of this one, one at a time.  The step's own kernel time
is what a kernel trace of leg (1) shows (`rocprofv3 --kernel-trace --stats -- python tools/gridsample_time.py --child nchw`); the figures here are
whole calls.  Without a usable GPU every leg fails.
usage (GPU box): python tools/gridsample_time.py"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.getcwd())

REPS, CALLS, ROWS, C, HW = 7, 25, 32, 64, (128, 128)
ELEMS = C * HW[0] * HW[1]
GRID = HW[0] * HW[1] * 2
THETA = np.array([0.98, -0.17, 0.02, 0.17, 0.98, -0.03], np.float32)


def line(tag, what, r, extra=""):
    print(f"{tag:<6} {what:<100} {ROWS} rows: median {r[0]:8.3f} ms a call (min {r[1]:8.3f}, max {r[2]:8.3f}, n={REPS} x {CALLS} calls) [{r[3]}]{extra}", flush=True)


def gbs(ms):
    return f"; {ROWS * (2 * ELEMS + GRID) * 4 / ms / 1e6:8.1f} GB/s of image read once + grid + result"


def torch_leg():
    import torch
    import torch.nn.functional as F

    if not torch.cuda.is_available():
        sys.exit(f"(3) torch-ROCm F.grid_sample: this torch build ({torch.__version__}) reports no usable GPU here")
    x = torch.rand((ROWS, C) + HW, device="cuda")
    g = F.affine_grid(torch.from_numpy(THETA).reshape(1, 2, 3).repeat(ROWS, 1, 1).cuda(), (ROWS, C) + HW, align_corners=False)
    for _ in range(2):
        F.grid_sample(x, g, mode="bilinear", padding_mode="zeros", align_corners=False)
    torch.cuda.synchronize()
    ts = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(CALLS):
            F.grid_sample(x, g, mode="bilinear", padding_mode="zeros", align_corners=False)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / CALLS)
    ts.sort()
    r = (ts[len(ts) // 2], ts[0], ts[-1], "resident NCHW float32")
    line("(3)", f"torch-ROCm F.grid_sample(x, grid), x {[C] + list(HW)}, grid {list(HW) + [2]}", r, gbs(r[0]))


def child(case):
    if case == "torch":
        return torch_leg()
    from infera_amd import capi, onnx_writer as W

    d = tempfile.mkdtemp()
    dev = capi.device_ordinal(0)

    def timed(name, blob, in_per_row, out_per_row, fill=None):
        capi.load_model(name, W.write(f"{d}/{name}.onnx", blob))
        d_in, d_out = capi.DeviceBuffer(dev, ROWS * in_per_row * 4), capi.DeviceBuffer(dev, ROWS * out_per_row * 4)
        if fill is None:
            capi.synth_fill(d_in, 42, 0, ROWS, in_per_row)
        else:
            d_in.upload(fill)
        capi.predict_device(name, d_in, ROWS, in_per_row, d_out)
        ms = sorted(capi.time_predict_device(name, d_in, ROWS, in_per_row, d_out, CALLS) / CALLS for _ in range(REPS))
        plan = capi.get_plan(name)
        what = "+".join(s["kind"] for s in plan["plan"]["steps"]) + " " + ",".join(f"{k['exec']} {k['in_layout']}->{k['out_layout']}" for k in plan.get("gridsample", []))
        capi.unload_model(name)
        del d_in, d_out
        return ms[len(ms) // 2], ms[0], ms[-1], what.strip()

    if case == "nchw":
        grid = (W.grid_sample_base(HW) @ THETA.reshape(2, 3)[:, :2].T + THETA.reshape(2, 3)[:, 2]).astype(np.float32)  # the rotation's grid
        rows = np.hstack([np.random.default_rng(1).uniform(-1, 1, size=(ROWS, ELEMS)).astype(np.float32), np.repeat(grid.reshape(1, -1), ROWS, axis=0)])
        r = timed("warp", W.grid_sample_model("grid", C, HW, HW), ELEMS + GRID, ELEMS, fill=np.ascontiguousarray(rows))
        line("(1)", "SliceCols(image) + SliceCols(grid) + GridSample, NCHW, a rotation by 10 degrees", r, gbs(r[0]))
        nodes = [W.node("Relu", ["X"], ["out"], name="relu")]
        e = timed("relu", W.model("eltwise", nodes, [], [W.value_info("X", ["N", C] + list(HW))], [W.value_info("out", ["N", C] + list(HW))]), ELEMS, ELEMS)
        line("(1)", "plain elementwise pass (Relu) over a buffer of the image's size", e, f"; {ROWS * ELEMS * 8 / e[0] / 1e6:8.1f} GB/s read plus written")
    elif case == "quads":
        base = timed("base", W.pixel_shuffle_model("crd", 1, C, HW, pre=True, post=True)[0], ELEMS, ELEMS)
        line("(2)", f"identity Conv 1x1 -> identity ConvTranspose 1x1 on [{C},{HW[0]},{HW[1]}]", base)
        r = timed("mid", W.grid_sample_model("affine", C, HW, HW, values=THETA, pre=True, post=True), ELEMS, ELEMS)
        line("(2)", "... with the localisation net and GridSample (affine) between them", r)
        print(f"(2)    the difference: {r[0] - base[0]:8.3f} ms{gbs(r[0] - base[0])}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    for case in ("nchw", "quads", "torch"):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", case], timeout=240)
        if p.returncode != 0:  # (a fault or a hang in one leg: nothing more is started on the GPU)
            sys.exit(f"leg {case} ended with status {p.returncode}")


if __name__ == "__main__":
    main()
