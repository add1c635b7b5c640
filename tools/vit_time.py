"""Times the Tokens step (hip/tokens.hip) and ViT-shaped models, device resident.
1. The step on the ViT-B/16 and ViT-Ti/16 token shapes (C = 768 / 192, S = 14 x 14, one class token, position table) read from NCHW: the
   model Relu + Tokens, the model Relu alone, and torch-ROCm's x.flatten(2).transpose(1, 2).contiguous() on a tensor of the same shape in
   the same process.  Two ratios to torch's time are printed: that of the whole Relu + Tokens model (an upper bound on the step's, the
   claim to check) and that of the difference of the two models (an ESTIMATE of the step alone, with its GB/s counted as 4 (C S + T E)
   bytes per image).  Read from channel quads (front = a 1x1 convolution) the step has no front that can be timed alone, so only the
   model's time is printed.
2. Whole models: a ViT-B/16-shaped one (224 x 224, E = 768, 12 layers, 12 heads, ff = 3072) and a ViT-Ti-shaped one (E = 192, 3 heads,
   ff = 768): images/s, and each step kind's share of the time.  The library has no per-step timer, so every kind is timed as a one-stage
   model on the model's own sizes (as tools/transformer_time.py does) and multiplied by the number of such steps in the plan; the shares
   are of the sum of those products, which is printed beside the whole model's time.
Every figure is the median of REPS windows after a warm call, each window long enough to last about WINDOW_MS; min and max are printed.
usage (GPU box): python tools/vit_time.py [--quick]      (--quick: the Ti shape only, fewer images)"""
import math
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.getcwd())
from infera_amd import capi, onnx_writer as W  # noqa: E402

REPS, WINDOW_MS = 7, 200.0


class T3:
    """median, min, max of the windows, in ms per call"""

    def __init__(self, ms):
        ms = sorted(ms)
        self.med, self.lo, self.hi = ms[len(ms) // 2], ms[0], ms[-1]

    def __str__(self):
        return f"median {self.med:8.3f} ms (min {self.lo:.3f}, max {self.hi:.3f}, n={REPS})"


def windows(per_window):
    """per_window(iters) -> ms for iters calls.  A short window sizes the timed ones."""
    iters = max(10, int(math.ceil(WINDOW_MS / max(per_window(10) / 10, 1e-4))))
    return T3([per_window(iters) / iters for _ in range(REPS)])


def run(name, blob, d, rows, cols, out_cols, dev):
    capi.load_model(name, W.write(f"{d}/{name}.onnx", blob))
    try:
        d_in, d_out = capi.DeviceBuffer(dev, rows * cols * 4), capi.DeviceBuffer(dev, rows * out_cols * 4)
        capi.synth_fill(d_in, 42, 0, rows, cols)
        capi.predict_device(name, d_in, rows, cols, d_out)
        return windows(lambda it: capi.time_predict_device(name, d_in, rows, cols, d_out, it)), capi.get_plan(name)
    finally:
        capi.unload_model(name)


def torch_copy(x):
    import torch

    fn = lambda: x.flatten(2).transpose(1, 2).contiguous()  # noqa: E731
    for _ in range(3):
        fn()
    torch.cuda.synchronize()

    def per_window(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    return windows(per_window)


def stage(nodes, inits, cols, out_dims):
    return W.model("stage", nodes, inits, [W.value_info("X", ["N", cols])], [W.value_info("out", out_dims)], opset=20)


def step_shapes(dev, d):
    import torch

    quick = "--quick" in sys.argv
    shapes = [("vit_ti", 192)] + ([] if quick else [("vit_b", 768)])
    print(f"Tokens step: bytes/s = 4 (C S + T E) bytes per image over the time; torch {torch.__version__}", flush=True)
    for label, E in shapes:
        hw, rows, S, T = (14, 14), (256 if quick else 1024), 196, 197
        byts = 4.0 * rows * (E * S + T * E)
        relu = W.model("front", [W.node("Relu", ["X"], ["front"])], [], [W.value_info("X", ["N", E] + list(hw))], [W.value_info("front", ["N", E] + list(hw))], opset=13)
        alone, _ = run(label + "_front", relu, d, rows, E * S, E * S, dev)
        both, plan = run(label + "_tok", W.tokens_model(E, hw, prefix=1, pos=True, front="relu")[0], d, rows, E * S, T * E, dev)
        assert plan["tokens"][0]["in_layout"] == "NCHW", plan["tokens"]
        x = torch.randn(rows, E, *hw, device="cuda")
        t = torch_copy(x)
        x = None
        head = f"{label} C={E} S={S} images={rows}"
        print(f"{head} Relu + Tokens (NCHW): {both}", flush=True)
        print(f"{head} Relu alone          : {alone}", flush=True)
        print(f"{head} torch x.flatten(2).transpose(1, 2).contiguous(): {t}  {8.0 * rows * E * S / t.med / 1e6:8.1f} GB/s (8 C S bytes per image)", flush=True)
        print(f"{head} ratio to torch's time: Relu + Tokens {both.med / t.med:5.3f} (range {both.lo / t.hi:5.3f} .. {both.hi / t.lo:5.3f}): an upper bound on the step's", flush=True)
        own = both.med - alone.med
        if own > 0:
            print(f"{head} Tokens alone, ESTIMATED as the difference of the two medians (the Relu's own store differs between the two models): "
                  f"~{own:8.3f} ms, ratio to torch {own / t.med:5.3f}, {byts / own / 1e6:8.1f} GB/s", flush=True)
        else:
            print(f"{head} Tokens alone: not separable, the difference of the two medians is not positive", flush=True)
        quads, plan = run(label + "_tokq", W.tokens_model(E, hw, prefix=1, pos=True, front="conv")[0], d, rows, E * S, T * E, dev)
        assert plan["tokens"][0]["in_layout"] == "NC/4HW4", plan["tokens"]
        print(f"{head} 1x1 Conv + Tokens (NC/4HW4): {quads} (no front to subtract: the convolution alone would store another layout)", flush=True)


def whole_models(dev, d):
    quick = "--quick" in sys.argv
    shapes = [("vit_ti", 192, 3, 768)] + ([] if quick else [("vit_b", 768, 12, 3072)])
    rng = np.random.default_rng(1)
    i64 = lambda name, v: W.tensor(name, np.asarray(v, dtype=np.int64))  # noqa: E731
    f32 = lambda name, v: W.tensor(name, np.asarray(v, dtype=np.float32))  # noqa: E731
    for label, E, h, ff in shapes:
        layers, rows, T = 12, (16 if quick else 64), 197
        spec = W.vit_spec(img=(3, 224, 224), patch=16, E=E, h=h, ff=ff, layers=layers, classes=1000, weight_scale=0.25)
        cols = 3 * 224 * 224
        whole, plan = run(label, W.vit_from_spec(spec), d, rows, cols, 1000, dev)
        kinds = [s["kind"] for s in plan["plan"]["steps"]]
        print(f"{label} whole model 224x224 E={E} L={layers} h={h}, {rows} images: {whole} = {rows / whole.med * 1e3:9.1f} images/s; {len(kinds)} steps", flush=True)
        # every step kind as a model of its own, on the model's sizes
        conv_attrs = [W.attr_ints("kernel_shape", [16, 16]), W.attr_ints("strides", [16, 16])]
        conv_inits = [W.tensor("patch_W", spec["patch_W"]), W.tensor("patch_b", spec["patch_b"])]
        nodes = [W.node("Conv", ["X", "patch_W", "patch_b"], ["patches"], conv_attrs)]
        conv, _ = run(label + "_conv", W.model("conv", nodes, conv_inits, [W.value_info("X", ["N", 3, 224, 224])], [W.value_info("patches", ["N", E, 14, 14])], opset=13), d, rows, cols, E * 196, dev)
        nodes, inits = [W.node("Conv", ["X", "patch_W", "patch_b"], ["patches"], conv_attrs)], list(conv_inits)
        out = W.token_nodes(nodes, inits, "patches", E, (14, 14), [spec["cls"]], spec["pos"])
        embed, _ = run(label + "_embed", W.model("embed", nodes, inits, [W.value_info("X", ["N", 3, 224, 224])], [W.value_info(out, ["N", T, E])], opset=13), d, rows, cols, T * E, dev)
        rs = lambda k: ([W.node("Reshape", ["X", "s"], ["x3"])], [i64("s", [-1, T, k])])  # noqa: E731

        def dense(tag, k, m):
            nodes, inits = rs(k)
            nodes += [W.node("MatMul", ["x3", "w"], ["mm"]), W.node("Add", ["mm", "b"], ["out"])]
            inits += [f32("w", rng.uniform(-1, 1, (k, m)) / np.sqrt(k)), f32("b", np.zeros(m))]
            return run(f"{label}_{tag}", stage(nodes, inits, T * k, ["N", T, m]), d, rows, T * k, T * m, dev)[0].med

        nodes, inits = rs(E)
        W.layernorm_nodes(nodes, inits, "x3", np.ones(E, np.float32), np.zeros(E, np.float32), "out", "ln", 1e-5, "op")
        ln = run(label + "_ln", stage(nodes, inits, T * E, ["N", T, E]), d, rows, T * E, T * E, dev)[0].med
        att = run(label + "_att", W.attention_only(T, E, h, form="packed"), d, rows, T * 3 * E, T * E, dev)[0].med
        nodes, inits = rs(E)
        relu = run(label + "_relu", stage(nodes + [W.node("Relu", ["x3"], ["out"])], inits, T * E, ["N", T, E]), d, rows, T * E, T * E, dev)[0].med
        nodes, inits = rs(E)
        radd = run(label + "_add", stage(nodes + [W.node("Relu", ["x3"], ["r"]), W.node("Add", ["r", "x3"], ["out"])], inits, T * E, ["N", T, E]), d, rows, T * E, T * E, dev)[0].med
        nodes, inits = rs(ff)
        gelu = run(label + "_gelu", stage(nodes + [W.node("Gelu", ["x3"], ["out"])], inits, T * ff, ["N", T, ff]), d, rows, T * ff, T * ff, dev)[0].med
        head = run(label + "_head", W.model("head", [W.node("MatMul", ["X", "w"], ["out"])], [f32("w", rng.uniform(-1, 1, (E, 1000)) / np.sqrt(E))],
                                           [W.value_info("X", ["N", E])], [W.value_info("out", ["N", 1000])], opset=20), d, rows, E, 1000, dev)[0].med
        per_kind = {
            "Conv2d": conv.med,
            "Tokens": max(embed.med - conv.med, 0.0),  # (an estimate: the convolution alone stores NCHW for the caller)
            "LayerNorm": kinds.count("LayerNorm") * ln,
            "Dense": layers * (dense("qkv", E, 3 * E) + dense("proj", E, E) + dense("ff1", E, ff) + dense("ff2", ff, E)) + head,
            "Attention": kinds.count("Attention") * att,
            "BinaryAct": kinds.count("BinaryAct") * max(radd - relu, 0.0),  # (the residual Add: Relu + Add minus Relu alone)
            "Unary": kinds.count("Unary") * gelu,
        }
        total = sum(per_kind.values())
        print(f"{label}   patch Conv alone {conv}; patch Conv + Tokens {embed}", flush=True)
        print(f"{label}   step kinds timed as one-stage models x their count in the plan: sum {total:9.3f} ms = {total / whole.med:5.3f} of the whole model's time "
              f"(SliceCols, one row per image, is not timed)", flush=True)
        for kind, ms in per_kind.items():
            print(f"{label}     {kind:<10} x{kinds.count(kind):>3}: {ms:9.3f} ms = {ms / total:6.1%} of the sum", flush=True)


def main():
    try:  # torch's ROCm runtime first (tools/transformer_time.py)
        import torch
        torch.cuda.is_available() and torch.zeros(1).cuda()
    except ImportError:
        pass
    d, dev = tempfile.mkdtemp(), capi.device_ordinal(0)
    step_shapes(dev, d)
    whole_models(dev, d)


if __name__ == "__main__":
    main()
