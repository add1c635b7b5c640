"""Times the Transformer-encoder steps (hip/attention.hip, hip/layernorm.hip, window Dense) on two shapes: a short window (T, F, E, h, ff, L) =
(24, 8, 64, 4, 256, 2) and a longer one (128, 128, 128, 8, 512, 2), both mean-pooled.  Per shape: the whole model device-resident (rows/s,
achieved f32 FLOP/s from flops_per_row against the f32 matrix-core peak) and every step kind alone as a one-stage model on the same sizes
(QKV projection, feed-forward pair, attention, LayerNorm with its GB/s against the streaming rate, the residual Add a fused LayerNorm would
save, mean over time, the Gelu operator beside its decomposed spelling, the operator LayerNorm beside the decomposed spelling on [N, T, E]);
REPS timed repetitions after a warm call, medians.  Then 16 callers end to end on 2048-row chunks, torch on 16 CPU threads, and the attention
step against torch's float32 scaled_dot_product_attention on the same tensors on the same GPU (CUDA events, same process).
usage (GPU box): python tools/transformer_time.py"""
import os
import sys
import tempfile
import threading
import time

import numpy as np

sys.path.insert(0, os.getcwd())
from infera_amd import capi, onnx_writer as W  # noqa: E402

PEAK, STREAM = 157.3e12, 6.3e12  # f32 MFMA vendor peak, achievable HBM streaming rate (profiles/r09_prep.txt)
REPS = 7
SHAPES = [("short_24x8_E64", 24, 8, 64, 4, 256, 2, 1 << 16), ("long_128_E128", 128, 128, 128, 8, 512, 2, 1 << 13)]


def i64(name, v):
    return W.tensor(name, np.asarray(v, dtype=np.int64))


def f32(name, v):
    return W.tensor(name, np.asarray(v, dtype=np.float32))


def stage(nodes, inits, cols, out_dims):
    return W.model("stage", nodes, inits, [W.value_info("X", ["N", cols])], [W.value_info("out", out_dims)], opset=20)


def timed(d, dev, name, blob, rows, cols, out_per_row, rng):
    """median ms of REPS device-resident calls"""
    capi.load_model(name, W.write(f"{d}/{name}.onnx", blob))
    x = rng.uniform(-1, 1, (rows, cols)).astype(np.float32)
    d_in, d_out = capi.DeviceBuffer(dev, x.nbytes), capi.DeviceBuffer(dev, rows * out_per_row * 4)
    d_in.upload(x)
    capi.predict_device(name, d_in, rows, cols, d_out)
    ms = sorted(capi.time_predict_device(name, d_in, rows, cols, d_out, 3) / 3 for _ in range(REPS))
    plan = capi.get_plan(name)
    capi.unload_model(name)
    del d_in, d_out
    return ms[len(ms) // 2], ms[0], ms[-1], plan


def line(tag, what, rows, med, lo, hi, extra=""):
    print(f"{tag:<16} {what:<44} {rows:>7} rows: median {med:8.3f} ms (min {lo:8.3f}, max {hi:8.3f}, n={REPS}) = {rows / med / 1e3:9.3f} M rows/s{extra}", flush=True)


def main():
    try:  # torch's ROCm runtime first: initialised after this library's contexts it reported no usable GPU in the same process
        import torch
        torch.cuda.is_available() and torch.zeros(1).cuda()
    except ImportError:
        pass
    d = tempfile.mkdtemp()
    dev = capi.device_ordinal(0)
    rng = np.random.default_rng(1)
    for tag, T, F, E, h, ff, L, rows in SHAPES:
        spec = W.transformer_spec(T=T, F=F, E=E, h=h, ff=ff, layers=L, act="Gelu")
        blob = W.transformer_from_spec(spec)
        med, lo, hi, plan = timed(d, dev, tag, blob, rows, T * F, 1, rng)
        flop = plan["plan"]["flops_per_row"]
        line(tag, "whole encoder (Gelu operator), mean-pooled", rows, med, lo, hi, f"; {flop} flop/row -> {rows * flop / med / 1e9:7.2f} TFLOP/s = {rows * flop / med * 1e3 / PEAK:5.3f} of the f32 MFMA peak")
        med2, lo2, hi2, _ = timed(d, dev, tag + "_dg", W.transformer_from_spec(spec, gelu="decomposed"), rows, T * F, 1, rng)
        line(tag, "whole encoder, decomposed GELU", rows, med2, lo2, hi2, f"; {med2 / med:5.3f} x the operator form")
        rs = lambda: [W.node("Reshape", ["X", "s"], ["x3"])]  # noqa: E731
        Wm = lambda k, m: (rng.uniform(-1, 1, (k, m)) / np.sqrt(k)).astype(np.float32)  # noqa: E731
        # QKV projection E -> 3E
        nodes = rs() + [W.node("MatMul", ["x3", "w"], ["mm"]), W.node("Add", ["mm", "b"], ["out"])]
        m, lo, hi, _ = timed(d, dev, tag + "_qkv", stage(nodes, [i64("s", [-1, T, E]), f32("w", Wm(E, 3 * E)), f32("b", np.zeros(3 * E))], T * E, ["N", T, 3 * E]), rows, T * E, T * 3 * E, rng)
        fl = 2 * T * E * 3 * E
        line(tag, f"window Dense {E}->{3 * E} (QKV)", rows, m, lo, hi, f"; {rows * fl / m / 1e9:7.2f} TFLOP/s = {rows * fl / m * 1e3 / PEAK:5.3f} of peak")
        # feed-forward pair
        nodes = rs() + [W.node("MatMul", ["x3", "w1"], ["m1"]), W.node("Add", ["m1", "b1"], ["a1"]), W.node("Relu", ["a1"], ["r1"]), W.node("MatMul", ["r1", "w2"], ["m2"]),
                        W.node("Add", ["m2", "b2"], ["out"])]
        inits = [i64("s", [-1, T, E]), f32("w1", Wm(E, ff)), f32("b1", np.zeros(ff)), f32("w2", Wm(ff, E)), f32("b2", np.zeros(E))]
        m, lo, hi, pl = timed(d, dev, tag + "_ff", stage(nodes, inits, T * E, ["N", T, E]), rows, T * E, T * E, rng)
        fl = 4 * T * E * ff
        line(tag, f"feed-forward {E}->{ff}->{E} ({'+'.join(sorted(set(pl['exec'])))})", rows, m, lo, hi, f"; {rows * fl / m / 1e9:7.2f} TFLOP/s = {rows * fl / m * 1e3 / PEAK:5.3f} of peak")
        # attention alone (packed input)
        m_att, lo, hi, _ = timed(d, dev, tag + "_att", W.attention_only(T, E, h, form="packed"), rows, T * 3 * E, T * E, rng)
        fl = 4 * T * T * E
        line(tag, f"Attention T={T} h={h} dh={E // h}", rows, m_att, lo, hi, f"; {rows * fl / m_att / 1e9:7.2f} TFLOP/s = {rows * fl / m_att * 1e3 / PEAK:5.3f} of peak")
        # LayerNorm, residual Add, mean over time: bytes moved = read + write
        g, b = np.ones(E, np.float32), np.zeros(E, np.float32)
        for what, form in (("LayerNorm operator", "op"), ("LayerNorm decomposed on [N,T,E] (existing passes)", "decomposed")):
            nodes, inits = rs(), [i64("s", [-1, T, E])]
            W.layernorm_nodes(nodes, inits, "x3", g, b, "out", "ln", 1e-5, form)
            m, lo, hi, pl = timed(d, dev, tag + "_ln" + form, stage(nodes, inits, T * E, ["N", T, E]), rows, T * E, T * E, rng)
            gb = rows * T * E * 8 / m / 1e6
            line(tag, f"{what} E={E} ({len(pl['plan']['steps'])} steps)", rows, m, lo, hi, f"; {gb:7.1f} GB/s of input + output = {gb * 1e9 / STREAM:5.3f} of 6.3 TB/s")
        nodes = rs() + [W.node("Relu", ["x3"], ["r"]), W.node("Add", ["r", "x3"], ["out"])]
        m, lo, hi, _ = timed(d, dev, tag + "_add", stage(nodes, [i64("s", [-1, T, E])], T * E, ["N", T, E]), rows, T * E, T * E, rng)
        nodes = rs() + [W.node("Relu", ["x3"], ["out"])]
        m1, _, _, _ = timed(d, dev, tag + "_relu", stage(nodes, [i64("s", [-1, T, E])], T * E, ["N", T, E]), rows, T * E, T * E, rng)
        line(tag, "residual Add pass (Relu+Add minus Relu alone)", rows, max(m - m1, 1e-6), lo - m1, hi - m1, "; what a LayerNorm with the Add fused would save per post-norm LayerNorm (not built)")
        nodes = rs() + [W.node("ReduceMean", ["x3", "ax"], ["out"], [W.attr_i("keepdims", 0)])]
        m, lo, hi, _ = timed(d, dev, tag + "_mean", stage(nodes, [i64("s", [-1, T, E]), i64("ax", [1])], T * E, ["N", E]), rows, T * E, E, rng)
        line(tag, "MeanTime", rows, m, lo, hi, f"; {rows * T * E * 4 / m / 1e6:7.1f} GB/s read")
        for what, dec in (("Gelu operator on [N,T,ff]", False), ("decomposed GELU on [N,T,ff]", True)):
            if dec:
                inits = [i64("s", [-1, T, ff]), f32("q", np.sqrt(2.0)), f32("one", 1.0), f32("half", 0.5)]
                nodes = [W.node("Reshape", ["X", "s"], ["x3"]), W.node("Div", ["x3", "q"], ["g0"]), W.node("Erf", ["g0"], ["g1"]), W.node("Add", ["g1", "one"], ["g2"]),
                         W.node("Mul", ["x3", "g2"], ["g3"]), W.node("Mul", ["g3", "half"], ["out"])]
            else:
                inits, nodes = [i64("s", [-1, T, ff])], [W.node("Reshape", ["X", "s"], ["x3"]), W.node("Gelu", ["x3"], ["out"])]
            m, lo, hi, pl = timed(d, dev, tag + "_gelu%d" % dec, stage(nodes, inits, T * ff, ["N", T, ff]), rows, T * ff, T * ff, rng)
            line(tag, f"{what} ({len(pl['plan']['steps'])} steps)", rows, m, lo, hi)
        # 16 callers end to end
        capi.load_model(tag, W.write(f"{d}/{tag}.onnx", blob))
        host_rows = 2048 * 48
        xh = rng.uniform(-1, 1, (host_rows, T * F)).astype(np.float32)
        chunks = [xh[i:i + 2048] for i in range(0, host_rows, 2048)]
        rates = []
        for _ in range(3):
            nxt, lock, ready = [0], threading.Lock(), threading.Barrier(17)

            def worker():
                capi.predict(tag, chunks[0])
                ready.wait()
                while True:
                    with lock:
                        i = nxt[0]
                        nxt[0] += 1
                    if i >= len(chunks):
                        return
                    capi.predict(tag, chunks[i])

            th = [threading.Thread(target=worker) for _ in range(16)]
            for t in th:
                t.start()
            ready.wait()
            t0 = time.perf_counter()
            for t in th:
                t.join()
            rates.append(host_rows / (time.perf_counter() - t0) / 1e6)
        print(f"{tag:<16} end to end, infera_predict, 16 callers x 2048-row chunks: {sorted(rates)[1]:7.3f} M rows/s (min {min(rates):.3f}, max {max(rates):.3f}, n=3)", flush=True)
        capi.unload_model(tag)
        try:
            import torch
        except ImportError:
            continue
        torch.set_num_threads(16)
        layer = torch.nn.TransformerEncoderLayer(E, h, ff, dropout=0.0, activation="gelu", batch_first=True)
        enc = torch.nn.TransformerEncoder(layer, L, enable_nested_tensor=False).eval()
        proj = torch.nn.Linear(F, E)
        n_cpu = 2048
        xt = torch.from_numpy(xh[:n_cpu].reshape(-1, T, F))
        with torch.no_grad():
            enc(proj(xt)).mean(1)
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                enc(proj(xt)).mean(1)
                ts.append(time.perf_counter() - t0)
        print(f"{tag:<16} torch-CPU float32, 16 threads, {n_cpu} rows (projection + encoder + mean): {n_cpu / sorted(ts)[1] / 1e6:7.4f} M rows/s (median of 3)", flush=True)
        if not torch.cuda.is_available():
            print(f"{tag:<16} torch-ROCm scaled_dot_product_attention: NOT MEASURED, this torch build ({torch.__version__}) reports no usable GPU here", flush=True)
            continue
        q, k, v = (torch.from_numpy(rng.uniform(-1, 1, (rows, h, T, E // h)).astype(np.float32)).cuda() for _ in range(3))
        F_ = torch.nn.functional
        for _ in range(3):
            F_.scaled_dot_product_attention(q, k, v)
        torch.cuda.synchronize()
        ts = []
        for _ in range(REPS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(3):
                F_.scaled_dot_product_attention(q, k, v)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) / 3)
        ts.sort()
        sd = ts[len(ts) // 2]
        print(f"{tag:<16} torch-ROCm float32 scaled_dot_product_attention, [N,h,T,dh] resident, {rows} rows: median {sd:8.3f} ms (min {ts[0]:.3f}, max {ts[-1]:.3f}, n={REPS}); "
              f"this kernel {m_att:8.3f} ms = {m_att / sd:5.2f} x torch's time", flush=True)
        del q, k, v
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
