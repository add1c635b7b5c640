"""Times the Rotary step (hip/rotary.hip) device-resident at the project's attention shape, 16,384 rows, T = 128, 8 heads x 16, and at that
shape with dh = 64.  Every attention model reads ONE packed input [N, T 3E] whose Split is absorbed, so the plans are Attention alone and
Rotary, Rotary, Attention: Q and K are rotated out of the packed rows where they lie.
  (1) the two Rotary steps' time: the model with rotary minus the same model without, medians, and the TB/s of their bytes read plus
      written (2 steps x 2 x N T E floats);
  (2) in the same process, the 3-D operator alone (one Rotary step over a dense [N, T, E] window, both pairings) and a plain elementwise pass
      of this project (Relu) over input and output buffers of the same size (every model gets fresh ones), in TB/s of 8 bytes per element;
  (3) torch-ROCm float32 evaluating Hugging Face's formula q * cos + rotate_half(q) * sin on resident [N, h, T, dh] tensors of the same shape
      (its own uniform values: the time does not depend on them), Q and K together, in a process of its own.
REPS timed windows of 3 calls after a warm call, medians; each leg is a child process of this one, one at a time.
usage (GPU box): python tools/rotary_time.py"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.getcwd())

REPS, ROWS, T, HQ = 7, 16384, 128, 8
SHAPES = (16, 64)  # dh


def eltwise_graph(W, e):
    nodes, inits = [W.node("Reshape", ["X", "s"], ["x3"]), W.node("Relu", ["x3"], ["out"], name="relu")], [W.tensor("s", np.asarray([-1, T, e], np.int64))]
    return W.model("eltwise", nodes, inits, [W.value_info("X", ["N", T * e])], [W.value_info("out", ["N", T, e])], opset=23)


def child(case, dh, tag):
    from infera_amd import capi, onnx_writer as W

    E = HQ * dh
    shape = f"T={T} h={HQ} dh={dh}"

    def line(what, r, extra=""):
        print(f"{tag:<8} {what:<66} {ROWS} rows: median {r[0]:8.3f} ms (min {r[1]:8.3f}, max {r[2]:8.3f}, n={REPS}) [{r[3]}]{extra}", flush=True)

    if case == "torch":
        import torch

        if not torch.cuda.is_available():
            print(f"{tag:<8} (3) torch-ROCm rotate_half formula: NOT MEASURED, this torch build ({torch.__version__}) reports no usable GPU here", flush=True)
            return
        g = torch.Generator(device="cuda").manual_seed(dh)
        q, k = (torch.rand((ROWS, HQ, T, dh), device="cuda", generator=g) * 2 - 1 for _ in range(2))
        cos, sin = (torch.from_numpy(np.concatenate([t, t], axis=1)).cuda() for t in W.rotary_tables(T, dh))

        def rope(t):
            return t * cos + torch.cat((-t[..., dh // 2:], t[..., : dh // 2]), dim=-1) * sin

        for _ in range(2):
            rope(q), rope(k)
        torch.cuda.synchronize()
        ts = []
        for _ in range(REPS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(3):
                rope(q), rope(k)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) / 3)
        ts.sort()
        r = (ts[len(ts) // 2], ts[0], ts[-1], "[N,h,T,dh] resident, Q and K")
        line(f"(3) torch-ROCm f32 x cos + rotate_half(x) sin, {shape}", r, f"; {ROWS * T * E * 4 * 4 / r[0] / 1e9:6.2f} TB/s of the 16 bytes per element a fused pass moves")
        return

    d = tempfile.mkdtemp()
    dev = capi.device_ordinal(0)

    def timed(name, blob, cols, out_per_row):
        capi.load_model(name, W.write(f"{d}/{name}.onnx", blob))
        d_in, d_out = capi.DeviceBuffer(dev, ROWS * cols * 4), capi.DeviceBuffer(dev, ROWS * out_per_row * 4)
        capi.synth_fill(d_in, 42, 0, ROWS, cols)
        capi.predict_device(name, d_in, ROWS, cols, d_out)
        ms = sorted(capi.time_predict_device(name, d_in, ROWS, cols, d_out, 3) / 3 for _ in range(REPS))
        steps = capi.get_plan(name)["plan"]["steps"]
        kinds = "+".join(s["kind"] + (":" + s["form"] if s["kind"] == "Rotary" else "") for s in steps)
        capi.unload_model(name)
        del d_in, d_out
        return ms[len(ms) // 2], ms[0], ms[-1], kinds

    if case == "model":
        plain = timed("plain", W.attention_op_model(T, T, HQ, HQ, dh, packed=True, causal=True), T * 3 * E, T * E)
        line(f"(1) Attention operator, is_causal, packed input, {shape}", plain)
        for rot in ({"form": "op"}, {"form": "slice"}):
            r = timed("rot_" + rot["form"], W.attention_op_model(T, T, HQ, HQ, dh, packed=True, causal=True, rotary=rot), T * 3 * E, T * E)
            line(f"(1) ... with rotary on Q and K ({'operator' if rot['form'] == 'op' else 'rotate_half spelling'}), {shape}", r)
            dt = r[0] - plain[0]
            print(f"{tag:<8} (1) the two Rotary steps: {dt:8.3f} ms = {dt / plain[0]:5.2f} of the Attention model; {ROWS * T * E * 4 * 4 / dt / 1e9:6.2f} TB/s of "
                  f"their bytes read plus written", flush=True)
    else:
        tb = lambda r: f"; {ROWS * T * E * 8 / r[0] / 1e9:6.2f} TB/s of 8 bytes per element"  # noqa: E731
        for inter in (False, True):
            r = timed(f"step{int(inter)}", W.rotary_model(T, HQ, dh, rotary={"interleaved": inter}), T * E, T * E)
            line(f"(2) Rotary step alone, {'interleaved' if inter else 'half'}, dense window, {shape}", r, tb(r))
        r = timed("step_scalar", W.rotary_model(T, HQ, dh, rotary={"rd": 2}), T * E, T * E)
        line(f"(2) Rotary step alone, half, rd = 2 (the scalar form), {shape}", r, tb(r))
        r = timed("relu", eltwise_graph(W, E), T * E, T * E)
        line(f"(2) plain elementwise pass (Relu), buffers of the same size, {shape}", r, tb(r))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default="")
    ap.add_argument("--dh", type=int, default=16)
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.dh, a.tag)
    for dh in SHAPES:
        for case in ("model", "step", "torch"):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", case, "--dh", str(dh), "--tag", f"dh={dh}"], timeout=420)
            if p.returncode != 0:  # (a fault or a hang in one leg: nothing more is started on the GPU)
                sys.exit(f"leg {case} dh={dh} ended with status {p.returncode}")


if __name__ == "__main__":
    main()
