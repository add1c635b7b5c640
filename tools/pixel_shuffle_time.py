"""Times the PixelShuffle step (hip/pixelshuffle.hip) device-resident at 64 -> 16 channels x 128^2 -> 256^2 with b = 2 (4 MiB per image on each
side), ROWS images a call.
  (1) NCHW to NCHW (pixelshuffle_generic): the model is the step alone, each of the four forms, in TB/s of its bytes read plus written, beside a
      plain elementwise pass of this project (Relu) over buffers of the same sizes in the same process;
  (2) channel quads to channel quads: DepthToSpace followed by the matching space-to-depth form between two identity 1x1 layers, minus the two
      identity layers alone: the two steps' time (pixelshuffle_quad_copy for DCR / SpaceToDepth, pixelshuffle_transpose for CRD /
      pixel_unshuffle), and the same with INFERA_PIXELSHUFFLE_FAST=0 (the generic form on channel quads);
  (3) the layout-crossing forms cannot be parted from the layer beside them by a subtraction, so they are timed as models, fast form beside
      generic form: identity Conv 1x1 -> DepthToSpace -> served NCHW (pixelshuffle_cq_to_nchw) and pixel_unshuffle of the caller's NCHW tensor
      -> identity ConvTranspose 1x1 (pixelshuffle_nchw_to_cq); the difference of a pair is the difference of the two kernel forms;
  (4) the ESPCN model of the writer (3 x 128 x 128 -> 3 x 256 x 256) per image, with the plan's layouts;
  (5) torch-ROCm's F.pixel_shuffle / F.pixel_unshuffle on resident [N, 64, 128, 128] / [N, 16, 256, 256] float32 tensors, in a process of its own.
REPS timed windows of 3 calls after a warm call, medians; each leg is a child process of this one, one at a time.
usage (GPU box): python tools/pixel_shuffle_time.py"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.getcwd())

REPS, ROWS, B, CS, HW = 7, 128, 2, 16, (128, 128)
C = CS * B * B
ELEMS = C * HW[0] * HW[1]  # per image, on either side of the step
DOWN = {"dcr": "s2d", "crd": "unshuffle"}


def line(tag, what, r, extra=""):
    print(f"{tag:<6} {what:<92} {ROWS} rows: median {r[0]:8.3f} ms (min {r[1]:8.3f}, max {r[2]:8.3f}, n={REPS}) [{r[3]}]{extra}", flush=True)


def tbs(ms, steps=1):
    return f"; {steps * ROWS * ELEMS * 8 / ms / 1e9:6.2f} TB/s of the bytes read plus written"


def torch_leg():
    import torch
    import torch.nn.functional as F

    if not torch.cuda.is_available():
        print(f"(5)    torch-ROCm F.pixel_shuffle: NOT MEASURED, this torch build ({torch.__version__}) reports no usable GPU here", flush=True)
        return
    for fn, shape, name in ((F.pixel_shuffle, (ROWS, C) + HW, "F.pixel_shuffle"), (F.pixel_unshuffle, (ROWS, CS, HW[0] * B, HW[1] * B), "F.pixel_unshuffle")):
        x = torch.rand(shape, device="cuda")
        for _ in range(2):
            fn(x, B)
        torch.cuda.synchronize()
        ts = []
        for _ in range(REPS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(3):
                fn(x, B)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) / 3)
        ts.sort()
        r = (ts[len(ts) // 2], ts[0], ts[-1], "resident NCHW float32")
        line("(5)", f"torch-ROCm {name}(x, {B}), {list(shape[1:])}", r, tbs(r[0]))


def child(case):
    if case == "torch":
        return torch_leg()
    from infera_amd import capi, onnx_writer as W

    d = tempfile.mkdtemp()
    dev = capi.device_ordinal(0)

    def timed(name, blob, in_per_row, out_per_row, fast=True, rows=ROWS):
        os.environ["INFERA_PIXELSHUFFLE_FAST"] = "1" if fast else "0"  # (read when a model is loaded)
        capi.load_model(name, W.write(f"{d}/{name}.onnx", blob))
        d_in, d_out = capi.DeviceBuffer(dev, rows * in_per_row * 4), capi.DeviceBuffer(dev, rows * out_per_row * 4)
        capi.synth_fill(d_in, 42, 0, rows, in_per_row)
        capi.predict_device(name, d_in, rows, in_per_row, d_out)
        ms = sorted(capi.time_predict_device(name, d_in, rows, in_per_row, d_out, 3) / 3 for _ in range(REPS))
        plan = capi.get_plan(name)
        what = "+".join(s["kind"] for s in plan["plan"]["steps"]) + " " + ",".join(f"{k['kernel']} {k['in_layout']}->{k['out_layout']}" for k in plan.get("pixelshuffle", []))
        capi.unload_model(name)
        del d_in, d_out
        return ms[len(ms) // 2], ms[0], ms[-1], what.strip()

    big = (CS, HW[0] * B, HW[1] * B)
    if case == "nchw":
        for form in ("dcr", "crd", "s2d", "unshuffle"):
            c, hw = (C, HW) if form in DOWN else (CS, big[1:])
            r = timed("alone_" + form, W.pixel_shuffle_model(form, B, c, hw, spelling=form == "unshuffle")[0], ELEMS, ELEMS)
            line("(1)", f"{form} alone, the caller's NCHW tensor to a served NCHW tensor", r, tbs(r[0]))
        nodes = [W.node("Relu", ["X"], ["out"], name="relu")]
        r = timed("relu", W.model("eltwise", nodes, [], [W.value_info("X", ["N", C] + list(HW))], [W.value_info("out", ["N", C] + list(HW))]), ELEMS, ELEMS)
        line("(1)", "plain elementwise pass (Relu), buffers of the same sizes", r, tbs(r[0]))
    elif case == "quads":
        base = timed("base", W.pixel_shuffle_model("crd", 1, C, HW, pre=True, post=True)[0], ELEMS, ELEMS)
        line("(2)", f"identity Conv 1x1 -> identity ConvTranspose 1x1 on [{C},{HW[0]},{HW[1]}] (no step: b = 1)", base)
        for form in DOWN:
            for fast in (True, False):
                r = timed(f"pair_{form}_{int(fast)}", W.pixel_shuffle_pair_model(form, B, C, HW, pre=True, post=True)[0], ELEMS, ELEMS, fast)
                line("(2)", f"... with {form} and {DOWN[form]} between them{'' if fast else ', INFERA_PIXELSHUFFLE_FAST=0'}", r)
                dt = r[0] - base[0]
                print(f"(2)    the two steps: {dt:8.3f} ms{tbs(dt, 2)}", flush=True)
    elif case == "crossing":
        for fast in (True, False):
            r = timed(f"out_{int(fast)}", W.pixel_shuffle_model("crd", B, C, HW, pre=True)[0], ELEMS, ELEMS, fast)
            line("(3)", f"identity Conv 1x1 -> crd -> served NCHW{'' if fast else ', INFERA_PIXELSHUFFLE_FAST=0'}", r)
        for fast in (True, False):
            r = timed(f"stem_{int(fast)}", W.pixel_shuffle_model("unshuffle", B, CS, big[1:], spelling=True, post=True)[0], ELEMS, ELEMS, fast)
            line("(3)", f"unshuffle of the caller's NCHW tensor -> identity ConvTranspose 1x1{'' if fast else ', INFERA_PIXELSHUFFLE_FAST=0'}", r)
    elif case == "espcn":
        blob, spec = W.espcn(b=B, size=HW[0], widths=(64, 32))
        r = timed("espcn", blob, 3 * HW[0] * HW[1], 3 * B * B * HW[0] * HW[1])
        line("(4)", f"ESPCN 3x{HW[0]}x{HW[1]} -> 3x{HW[0] * B}x{HW[1] * B} (conv 5x5 to 64, 3x3 to 32, 3x3 to {3 * B * B}, PixelShuffle)", r,
             f"; {r[0] / ROWS * 1e3:7.1f} us per image, {ROWS / r[0] * 1e3:8.0f} images/s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    for case in ("nchw", "quads", "crossing", "espcn", "torch"):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", case], timeout=240)
        if p.returncode != 0:  # (a fault or a hang in one leg: nothing more is started on the GPU)
            sys.exit(f"leg {case} ended with status {p.returncode}")


if __name__ == "__main__":
    main()
