"""Times attention under per-row key masks (hip/attention.hip attention_kernel<DT, true>) and the masked mean over time, device-resident,
16,384 rows, at T = 128, h = 8, dh = 16 and T = 128, h = 4, dh = 64.  Every model reads the same table [packed q|k|v window, T mask columns],
so every plan is SliceCols + Attention and the plans differ in the attention step alone:
  (a) the unmasked model, on a build of the parent commit (--parent-lib) and on this one, alternating, twice each;
  (b) the masked model (add, finfo.min), every key kept;
  (c) lengths uniform in 8 .. 128 (right-padded);
  (d) every row of length 16;
  (e) (c) with INFERA_ATTN_SKIP=0: every tile visited;
  (f) torch-ROCm float32 scaled_dot_product_attention with the boolean mask of (c) on the same tensors;
and the masked MeanTime (T = 128, E = 128, lengths as in (c)) beside the plain one.  A library is chosen when a process starts
(INFERA_LIB_PATH) and INFERA_ATTN_SKIP is read once per process, so each leg is a child process of this one, one at a time; REPS timed
repetitions of 3 calls after a warm call, medians.
usage (GPU box): python tools/padded_time.py [--parent-lib ab/parent/libinfera.so]"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.getcwd())

REPS, ROWS, T = 7, 16384, 128
SHAPES = [(8, 16), (4, 64)]  # (h, dh)
FMIN = float(np.finfo(np.float32).min)


def graphs(W, E, h, masked):
    """attention alone over inputs X [N, T 3E] and M [N, T] (int64); the unmasked model ignores M"""
    nodes = [W.node("Reshape", ["X", "x_shape"], ["X3"]), W.node("Split", ["X3", "sp"], ["q", "k", "v"], [W.attr_i("axis", 2)], name="split_qkv")]
    inits = [W.tensor("x_shape", np.asarray([-1, T, 3 * E], dtype=np.int64)), W.tensor("sp", np.asarray([E, E, E], dtype=np.int64))]
    out = W.attention_nodes(nodes, inits, "a_", "q", "k", "v", "X3", T, E, h, **({"row_mask": dict(src="M", form="add", fill=FMIN)} if masked else {}))
    return W.model("attention", nodes, inits, [W.value_info("X", ["N", T * 3 * E]), W.value_info("M", ["N", T], W.INT64)], [W.value_info(out, ["N", T, E])], opset=20)


def mean_graph(W, E, masked):
    nodes, inits = [W.node("Reshape", ["X", "s"], ["x3"])], [W.tensor("s", np.asarray([-1, T, E], np.int64))]
    if masked:
        out = W.masked_mean_nodes(nodes, inits, "mm_", "x3", "M", T, E)
    else:
        inits.append(W.tensor("ax", np.asarray([1], np.int64)))
        nodes.append(W.node("ReduceMean", ["x3", "ax"], ["out"], [W.attr_i("keepdims", 0)]))
        out = "out"
    return W.model("mean", nodes, inits, [W.value_info("X", ["N", T * E]), W.value_info("M", ["N", T], W.INT64)], [W.value_info(out, ["N", E])], opset=20)


def lengths(kind, rng):
    if kind == "all":
        return np.full(ROWS, T)
    if kind == "len16":
        return np.full(ROWS, 16)
    return rng.integers(8, T + 1, ROWS)


def child(cases, tag):
    from infera_amd import capi, onnx_writer as W

    torch = None
    if "f" in cases:  # torch's ROCm runtime first (tools/transformer_time.py)
        import torch
        torch.cuda.is_available() and torch.zeros(1).cuda()
    d = tempfile.mkdtemp()
    dev = capi.device_ordinal(0)

    def timed(name, blob, x, out_per_row):
        capi.load_model(name, W.write(f"{d}/{name}.onnx", blob))
        d_in, d_out = capi.DeviceBuffer(dev, x.nbytes), capi.DeviceBuffer(dev, ROWS * out_per_row * 4)
        d_in.upload(x)
        capi.predict_device(name, d_in, ROWS, x.shape[1], d_out)
        ms = sorted(capi.time_predict_device(name, d_in, ROWS, x.shape[1], d_out, 3) / 3 for _ in range(REPS))
        kinds = "+".join(s["kind"] for s in capi.get_plan(name)["plan"]["steps"])
        capi.unload_model(name)
        del d_in, d_out
        return ms[len(ms) // 2], ms[0], ms[-1], kinds

    def line(what, r, extra=""):
        print(f"{tag:<18} {what:<58} {ROWS} rows: median {r[0]:8.3f} ms (min {r[1]:8.3f}, max {r[2]:8.3f}, n={REPS}) [{r[3]}]{extra}", flush=True)

    for h, dh in SHAPES:
        E = h * dh
        rng = np.random.default_rng(E)
        x = np.empty((ROWS, T * 3 * E + T), np.float32)
        x[:, :T * 3 * E] = rng.random((ROWS, T * 3 * E), dtype=np.float32) * 2 - 1
        shape = f"T={T} h={h} dh={dh}"
        for case, kind, masked in (("a", "all", False), ("b", "all", True), ("c", "uniform", True), ("d", "len16", True)):
            if case not in cases:
                continue
            L = lengths(kind, np.random.default_rng(7))
            x[:, T * 3 * E:] = np.arange(T)[None, :] < L[:, None]
            what = {"a": "(a) unmasked", "b": "(b) masked, every key kept", "c": "(c) masked, lengths uniform in 8..128", "d": "(d) masked, every row of length 16"}[case]
            if case == "c" and os.environ.get("INFERA_ATTN_SKIP") == "0":
                what = "(e) = (c) with INFERA_ATTN_SKIP=0"
            line(f"{what}, {shape}", timed(f"att_{case}_{E}", graphs(W, E, h, masked), x, T * E), f"; mean length {L.mean():.1f}")
        if "f" in cases:
            if not torch.cuda.is_available():
                print(f"{tag:<18} (f) torch-ROCm scaled_dot_product_attention: NOT MEASURED, this torch build ({torch.__version__}) reports no usable GPU here", flush=True)
            else:
                L = lengths("uniform", np.random.default_rng(7))
                qkv = torch.from_numpy(x[:, :T * 3 * E].reshape(ROWS, T, 3, h, dh)).cuda()
                q, k, v = (qkv[:, :, j].permute(0, 2, 1, 3).contiguous() for j in range(3))
                del qkv
                mask = torch.from_numpy(np.arange(T)[None, :] < L[:, None]).cuda()[:, None, None, :]
                F_ = torch.nn.functional
                for _ in range(3):
                    F_.scaled_dot_product_attention(q, k, v, attn_mask=mask)
                torch.cuda.synchronize()
                ts = []
                for _ in range(REPS):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(3):
                        F_.scaled_dot_product_attention(q, k, v, attn_mask=mask)
                    e1.record()
                    torch.cuda.synchronize()
                    ts.append(e0.elapsed_time(e1) / 3)
                ts.sort()
                line(f"(f) torch-ROCm f32 SDPA, bool mask of (c), {shape}", (ts[len(ts) // 2], ts[0], ts[-1], "[N,h,T,dh] resident, no SliceCols"))
                del q, k, v, mask
                torch.cuda.empty_cache()
        del x
    if "m" in cases:
        E = 128
        rng = np.random.default_rng(3)
        x = np.empty((ROWS, T * E + T), np.float32)
        x[:, :T * E] = rng.random((ROWS, T * E), dtype=np.float32) * 2 - 1
        L = lengths("uniform", np.random.default_rng(7))
        x[:, T * E:] = np.arange(T)[None, :] < L[:, None]
        for what, masked in (("MeanTime, plain", False), ("MeanTime with a row mask, lengths uniform in 8..128", True)):
            r = timed(f"mean{int(masked)}", mean_graph(W, E, masked), x, E)
            line(f"{what}, T={T} E={E}", r, f"; {ROWS * T * E * 4 / r[0] / 1e6:7.1f} GB/s of the window")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default="ab/parent/libinfera.so")
    ap.add_argument("--child", default="")
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.tag)

    def leg(cases, tag, **env):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", cases, "--tag", tag], env=dict(os.environ, **env), timeout=900)
        if p.returncode != 0:  # (a fault or a hang in one leg: nothing more is started on the GPU)
            sys.exit(f"leg {tag} ended with status {p.returncode}")

    if os.path.exists(a.parent_lib):
        for i in range(2):
            leg("a", f"parent run {i + 1}", INFERA_LIB_PATH=os.path.abspath(a.parent_lib))
            leg("a", f"this run {i + 1}")
    else:
        print(f"(a) on the parent commit: NOT MEASURED, {a.parent_lib} is missing (build the parent commit's libinfera.so there)", flush=True)
        leg("a", "this run 1")
        leg("a", "this run 2")
    leg("bcdfm", "this")
    leg("c", "this, no skipping", INFERA_ATTN_SKIP="0")


if __name__ == "__main__":
    main()
