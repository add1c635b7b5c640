"""Times the Interact kernels (hip/interact.hip), device resident, 131,072 rows: DLRM's pairwise dots at k = 27, d = 16 and k = 27, d = 128
(the strict lower triangle, 351 products; the Criteo shape) and the FM bi-interaction term at k = 39, d = 10.
The step is timed as a model minus the same model without the step, so its rows are ESTIMATES:
    plain         T is the model input: (Interact -> Relu) - (Relu alone on the [N, F] result)
    pass-through  T = Concat(x [N, d], rest): (Concat -> Interact with x passed through -> Relu) - ((Concat -> Relu) - Relu on [N, k d]) - Relu on [N, F]
Per shape: the step's ms, its bytes/s over 4 * (k d + F) bytes per row (T read once, the row written), a plain elementwise pass (Relu alone)
over as many bytes in the same run, the fraction of the fp32 matrix bound (the flops the tiles issue, 2 * tile^2 * d rounded up to the
k-step group, at 157.3 TFLOP/s) and torch-ROCm float32 on the same tensors on the same GPU: bmm + index (+ cat) for dot, the written
formula for fm.  Medians of 5 windows of 20 passes.
(profiles/r21_interact.txt also holds the A/B of the two epilogues, taken with the scattered-store variant before it was removed.)
usage (GPU box): python tools/interact_time.py [--quick]      (--quick: 8x fewer rows)"""
import os
import statistics
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.getcwd())
from infera_amd import capi, onnx_writer as W  # noqa: E402

REPS, WINDOWS = 20, 5
MFMA_F32 = 157.3e12


def timed(name, blob, d, rows, cols, out_cols, dev):
    capi.load_model(name, W.write(f"{d}/{name}.onnx", blob))
    try:
        d_in, d_out = capi.DeviceBuffer(dev, rows * cols * 4), capi.DeviceBuffer(dev, rows * out_cols * 4)
        capi.synth_fill(d_in, 42, 0, rows, cols)
        capi.predict_device(name, d_in, rows, cols, d_out)
        ms = statistics.median(capi.time_predict_device(name, d_in, rows, cols, d_out, REPS) / REPS for _ in range(WINDOWS))
        return ms, capi.get_plan(name)
    finally:
        capi.unload_model(name)


def relu_alone(flat):
    return W.model("relu", [W.node("Relu", ["X"], ["Y"], name="tail")], [], [W.value_info("X", ["N", flat])], [W.value_info("Y", ["N", flat])])


def dot_model(k, d, sel, passing, step=True):
    """plain: X [N, k d] -> Reshape -> T.  passing: inputs x [N, d] and rest [N, (k - 1) d] -> Concat -> Reshape -> T, and the result is
    cat([x, Zsel], 1).  step = False (passing only): the Concat and a Relu of T, nothing else"""
    nodes, inits = [], [W.tensor("window_shape", np.asarray([-1, k, d], dtype=np.int64))]
    if passing:
        inputs = [W.value_info("x", ["N", d]), W.value_info("rest", ["N", (k - 1) * d])]
        nodes.append(W.node("Concat", ["x", "rest"], ["X"], [W.attr_i("axis", 1)], name="join"))
    else:
        inputs = [W.value_info("X", ["N", k * d])]
    if not step:
        nodes.append(W.node("Relu", ["X"], ["Y"], name="tail"))
        return W.model("front", nodes, [], inputs, [W.value_info("Y", ["N", k * d])]), k * d
    nodes.append(W.node("Reshape", ["X", "window_shape"], ["T"], name="window"))
    cur, dims = W.interact_dot_nodes(nodes, inits, "T", k, "gather", sel)
    F = dims[0]
    if passing:
        nodes.append(W.node("Concat", ["x", cur], ["R"], [W.attr_i("axis", 1)], name="cat_r"))
        cur, F = "R", F + d
    nodes.append(W.node("Relu", [cur], ["Y"], name="tail"))
    return W.model("dot", nodes, inits, inputs, [W.value_info("Y", ["N", F])]), F


def fm_model(k, d):
    nodes, inits, T, inputs, _ = W.interact_window_nodes(k, d, "reshape")
    cur, dims = W.interact_fm_nodes(nodes, inits, T, d, h=0.5)
    nodes.append(W.node("Relu", [cur], ["Y"], name="tail"))
    return W.model("fm", nodes, inits, inputs, [W.value_info("Y", ["N", d])]), d


def torch_ms(fn):
    import torch

    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(WINDOWS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(REPS):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / REPS)
    return statistics.median(out)


def report(label, rows, own, k, d, F, plain_ms, plain_floats, issued_flops):
    step_bytes = 4.0 * (k * d + F) * rows
    plain_rate = 8.0 * plain_floats * rows / plain_ms / 1e9
    line = f"{label:<34} rows={rows:>7} step~{own:8.4f} ms  {step_bytes / own / 1e9:7.3f} TB/s over {4 * (k * d + F)} B/row  (plain pass over as many bytes {plain_ms:8.4f} ms, {plain_rate:6.3f} TB/s)"
    if issued_flops:
        line += f"  matrix bound {issued_flops * rows / MFMA_F32 * 1e3:7.4f} ms = {issued_flops * rows / MFMA_F32 * 1e3 / own:5.3f} of the step"
    print(line, flush=True)


def main():
    import torch

    quick = "--quick" in sys.argv
    tmp = tempfile.mkdtemp()
    dev = capi.device_ordinal(0)
    rows = 131072 // (8 if quick else 1)
    print(f"the step's time = a model's minus the same model without the step (estimates); torch {torch.__version__}", flush=True)
    g = torch.device("cuda:0") if torch.cuda.is_available() else None
    for k, d in ((27, 16), (27, 128)):
        sel = W.interact_triangle(k)
        tile = 16 if k <= 16 else 32 if k <= 32 else 64
        group = 16 if tile == 16 else 8
        issued = 2.0 * tile * tile * ((d + group - 1) // group * group)
        # plain
        blob, F = dot_model(k, d, sel, False)
        ms, plan = timed("dot", blob, tmp, rows, k * d, F, dev)
        assert [s["kind"] for s in plan["plan"]["steps"]] == ["Interact", "Unary"], plan["plan"]["steps"]
        relu_f, _ = timed("relu", relu_alone(F), tmp, rows, F, F, dev)
        half = (k * d + F) // 2
        plain_ms, _ = timed("relu", relu_alone(half), tmp, rows, half, half, dev)
        own = ms - relu_f
        report(f"dot k={k} d={d} triangle P={len(sel)}", rows, own, k, d, F, plain_ms, half, issued)
        # pass-through
        blob, Fp = dot_model(k, d, sel, True)
        msp, plan = timed("dotp", blob, tmp, rows, k * d, Fp, dev)
        kinds = [s["kind"] for s in plan["plan"]["steps"]]
        assert kinds.count("Interact") == 1 and kinds[-2:] == ["Interact", "Unary"], kinds
        ia = [s for s in plan["plan"]["steps"] if s["kind"] == "Interact"][0]
        assert ia["pass_through"] == [{"src": 0, "len": d, "out": 0}], ia
        front, _ = timed("front", dot_model(k, d, sel, True, step=False)[0], tmp, rows, k * d, k * d, dev)
        relu_kd, _ = timed("relu", relu_alone(k * d), tmp, rows, k * d, k * d, dev)
        relu_fp, _ = timed("relu", relu_alone(Fp), tmp, rows, Fp, Fp, dev)
        ownp = msp - (front - relu_kd) - relu_fp
        halfp = (k * d + Fp) // 2
        plainp_ms, _ = timed("relu", relu_alone(halfp), tmp, rows, halfp, halfp, dev)
        report(f"dot k={k} d={d} triangle + pass-through", rows, ownp, k, d, Fp, plainp_ms, halfp, issued)
        if g is None:
            print("torch: no GPU visible to torch", flush=True)
            continue
        T = torch.randn(rows, k, d, device=g)
        li = torch.tensor([i for i in range(k) for j in range(i)], device=g)
        lj = torch.tensor([j for i in range(k) for j in range(i)], device=g)
        t1 = torch_ms(lambda: torch.bmm(T, T.transpose(1, 2))[:, li, lj])
        t2 = torch_ms(lambda: torch.cat([T[:, 0], torch.bmm(T, T.transpose(1, 2))[:, li, lj]], dim=1))
        print(f"{'':<34} torch-ROCm f32 bmm + index {t1:8.4f} ms (step / torch = {own / t1:5.3f});  bmm + index + cat {t2:8.4f} ms (step / torch = {ownp / t2:5.3f})", flush=True)
        del T
        torch.cuda.empty_cache()
    k, d = 39, 10
    blob, F = fm_model(k, d)
    ms, plan = timed("fm", blob, tmp, rows, k * d, F, dev)
    assert [s["kind"] for s in plan["plan"]["steps"]] == ["Interact", "Unary"], plan["plan"]["steps"]
    relu_f, _ = timed("relu", relu_alone(F), tmp, rows, F, F, dev)
    half = (k * d + F) // 2
    plain_ms, _ = timed("relu", relu_alone(half), tmp, rows, half, half, dev)
    own = ms - relu_f
    report(f"fm k={k} d={d} h=0.5", rows, own, k, d, F, plain_ms, half, 0)
    if g is not None:
        T = torch.randn(rows, k, d, device=g)

        def written():
            s = T.sum(dim=1)
            return 0.5 * (s * s - (T * T).sum(dim=1))

        t = torch_ms(written)
        print(f"{'':<34} torch-ROCm f32, the written formula {t:8.4f} ms (step / torch = {own / t:5.3f})", flush=True)


if __name__ == "__main__":
    main()
