"""Times the Embed kernel (hip/embed.hip), device resident, on three shapes: 26 tables x d 16 + 13 numeric columns (the Criteo layout, spelling
(a)), 8 columns x d 32 out of one shared table with offsets (spelling (b), window form) and T = 128 token ids into a 30,522 x 256 table
(spelling (c)).  The step is timed as a model (Embed -> Relu) minus the same model fed the already-embedded row (the Relu alone, on buffers of
the same sizes), so its rows are ESTIMATES.  Per shape: the step's ms per pass, its bytes/s counted as 4 * (source columns + gathered floats +
written floats) per row, beside the plain elementwise pass (the Relu alone: one read and one write per element) on the same run; then
torch-ROCm's F.embedding + cat on the same tensors on the same GPU.  Medians of 5 windows of 20 passes.
usage (GPU box): python tools/embed_time.py [--quick]      (--quick: 8x fewer rows)"""
import os
import statistics
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.getcwd())
from infera_amd import capi, onnx_writer as W  # noqa: E402

REPS, WINDOWS = 20, 5


def timed(name, blob, d, x, rows, cols, out_cols, dev):
    """median ms per pass of the model `blob` on x (a host array [rows, cols], or None: synthetic floats), and its plan"""
    capi.load_model(name, W.write(f"{d}/{name}.onnx", blob))
    try:
        d_in, d_out = capi.DeviceBuffer(dev, rows * cols * 4), capi.DeviceBuffer(dev, rows * out_cols * 4)
        if x is None:
            capi.synth_fill(d_in, 42, 0, rows, cols)
        else:
            d_in.upload(x)
        capi.predict_device(name, d_in, rows, cols, d_out)
        ms = statistics.median(capi.time_predict_device(name, d_in, rows, cols, d_out, REPS) / REPS for _ in range(WINDOWS))
        return ms, capi.get_plan(name)
    finally:
        capi.unload_model(name)


def with_relu(front):
    nodes, inits, cur, dims, inputs = front
    flat = int(np.prod(dims[1:]))
    return W.model("embed_relu", nodes + [W.node("Relu", [cur], ["Y"], name="tail")], inits, inputs, [W.value_info("Y", dims)]), flat


def relu_alone(flat):
    return W.model("relu", [W.node("Relu", ["X"], ["Y"], name="tail")], [], [W.value_info("X", ["N", flat])], [W.value_info("Y", ["N", flat])])


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


def main():
    import torch
    import torch.nn.functional as F

    quick = "--quick" in sys.argv
    d = tempfile.mkdtemp()
    dev = capi.device_ordinal(0)
    print(f"step = (Embed -> Relu) - (Relu alone on the embedded row), an estimate; step bytes = 4 * (source + gathered + written floats) per row; "
          f"plain pass bytes = 8 per element; torch {torch.__version__}", flush=True)
    shapes = (("criteo 26 x d16 + 13", "a", dict(cards=(40000,) * 26, dims=16, numeric=13), {}, 131072),
              ("shared 8 x d32 window", "b", dict(cards=(20000,) * 8, dims=32, numeric=0), {"flatten": "window"}, 262144),
              ("tokens T128 30522 x 256", "c", dict(cards=(30522,) * 128, dims=256, numeric=0), {}, 2048))
    for label, spelling, kw, front_kw, rows in shapes:
        rows = rows // 8 if quick else rows
        if spelling == "c":  # (one table: the spec's other 127 are never built)
            spec = W.embedding_spec(cards=kw["cards"][:1], dims=kw["dims"], numeric=0, hidden=())
            spec["cards"], spec["dims"] = list(kw["cards"]), [kw["dims"]] * len(kw["cards"])
        else:
            spec = W.embedding_spec(hidden=(), **kw)
        x_cat, x_num, x = W.embedding_inputs(spec, rows, seed=1, spelling=spelling)
        blob, flat = with_relu(W.embedding_nodes(spec, spelling, **front_kw))
        cols = x.shape[1]
        ms, plan = timed("embed", blob, d, x, rows, cols, flat, dev)
        step = plan["plan"]["steps"][0]
        assert [s["kind"] for s in plan["plan"]["steps"]] == ["Embed", "Unary"], plan["plan"]["steps"]
        base, _ = timed("relu", relu_alone(flat), d, None, rows, flat, flat, dev)
        own = ms - base
        step_bytes, plain_bytes = float(step["bytes_per_row"]) * rows, 8.0 * rows * flat
        print(f"{label:<24} rows={rows:>7} F'={flat:>6} model {ms:8.3f} ms  Relu alone {base:8.3f} ms ({plain_bytes / base / 1e6:7.1f} GB/s)  step~{own:8.3f} ms  "
              f"{step_bytes / own / 1e6:7.1f} GB/s  = {(step_bytes / own) / (plain_bytes / base):5.3f} of the plain pass's rate  (rows per tile {step['rows_per_tile']})", flush=True)
        if not torch.cuda.is_available():
            print(f"{label:<24} torch: no GPU visible to torch", flush=True)
            continue
        g = torch.device("cuda:0")
        idx = torch.from_numpy(x_cat).to(g)
        if spelling == "a":
            tabs = [torch.from_numpy(t).to(g) for t in spec["tables"]]
            num = torch.from_numpy(x_num).to(g)
            fn = lambda: torch.cat([F.embedding(idx[:, j], tabs[j]) for j in range(len(tabs))] + [num], dim=1)  # noqa: E731
        elif spelling == "b":
            tab, off = torch.from_numpy(spec["shared"]).to(g), torch.from_numpy(spec["offsets"]).to(g)
            fn = lambda: F.embedding(idx + off, tab)  # noqa: E731
        else:
            tab = torch.from_numpy(spec["tables"][0]).to(g)
            fn = lambda: F.embedding(idx, tab)  # noqa: E731
        t = torch_ms(fn)
        print(f"{label:<24} torch-ROCm F.embedding{' + cat' if spelling == 'a' else ''}, the same tensors on the same GPU rows={rows:>7} {t:8.3f} ms  "
              f"{step_bytes / t / 1e6:7.1f} GB/s (same byte count)  step / torch = {own / t:5.3f}", flush=True)
        del idx, fn
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
