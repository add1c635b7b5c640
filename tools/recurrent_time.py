"""Times the recurrent kernel (hip/rnn.hip) on three shapes: LSTM (T, F, H) = (24, 8, 64), GRU (96, 4, 128) two layers bidirectional and LSTM
(256, 16, 64), each serving the whole sequence from a flat [rows, T*F] table.  Per shape, REPS timed repetitions (HIP events on the launching
stream, after a warm call) of a device-resident scan and of one 2048-row chunk; the fraction of the f32 matrix-core peak from
2 T D G H (F + H) flop per row, the fraction of HBM from the bytes the plan must move (input once, every step's output once, every
intermediate written and read once), which of the two bounds the shape; end to end through infera_predict with 16 callers on 2048-row chunks;
and torch on the CPU in float32 with 16 threads.

--lens PATTERN [PATTERN ...] times per-row sequence_lens instead (INTEGRATION.md 2.6 "Padded windows"), device-resident, 131,072 rows, on
LSTM 24 x 8, H = 64 (the README's case) and GRU 96 x 4, H = 128, two layers, bidirectional, Y_h served: first the fixed-length model, then
the same model with a length column under each pattern:
  full            every length = T: what the feature costs when nothing is padded
  quarter         every length = T / 4
  uniform         lengths uniform in 1 .. T, rows in random order: every 16-row tile runs to its longest row, near T
  uniform-sorted  the same lengths sorted: a tile runs the steps its rows have
--runs N repeats every measurement N times (default 5; each is the median of REPS timings of 3 passes) to show the run-to-run spread.
--fixed-only times the fixed-length model alone (for a build without the feature: INFERA_LIB_PATH chooses the library).
usage (GPU box): python tools/recurrent_time.py [--lens full quarter uniform uniform-sorted] [--runs 5] [--fixed-only]"""
import argparse
import os
import sys
import tempfile
import threading
import time

import numpy as np

sys.path.insert(0, os.getcwd())
from infera_amd import capi, onnx_writer as W  # noqa: E402

PEAK, HBM = 157.3e12, 8.0e12  # f32 MFMA and HBM3E, vendor peaks
REPS = 7
SHAPES = [  # name, op, T, F, H, layers, direction, resident rows
    ("lstm_24x8x64", "LSTM", 24, 8, 64, 1, "forward", 1 << 20),
    ("gru_96x4x128_2l_bi", "GRU", 96, 4, 128, 2, "bidirectional", 1 << 17),
    ("lstm_256x16x64", "LSTM", 256, 16, 64, 1, "forward", 1 << 17),
]


def spread(v):
    v = sorted(v)
    return f"median {v[len(v) // 2]:9.3f} ms (min {v[0]:9.3f}, max {v[-1]:9.3f}, n={len(v)})"


LENS_SHAPES = [("lstm_24x8x64", "LSTM", 24, 8, 64, 1, "forward"), ("gru_96x4x128_2l_bi", "GRU", 96, 4, 128, 2, "bidirectional")]
LENS_ROWS = 131072


def lens_column(pattern, T, rows, rng):
    if pattern == "full":
        return np.full(rows, T)
    if pattern == "quarter":
        return np.full(rows, max(T // 4, 1))
    ln = rng.integers(1, T + 1, rows)
    return np.sort(ln) if pattern == "uniform-sorted" else ln


def lens_main(patterns, runs, fixed_only):
    d = tempfile.mkdtemp()
    dev = capi.device_ordinal(0)
    rows = LENS_ROWS
    for name, op, T, F, H, layers, direction in LENS_SHAPES:
        spec = W.recurrent_spec(op, T=T, F=F, H=H, layers=layers, direction=direction)
        D = spec["D"]
        rng = np.random.default_rng(1)
        x = rng.normal(0, 1, (rows, T * F)).astype(np.float32)
        d_out = capi.DeviceBuffer(dev, rows * D * H * 4)

        def timed(model, table, label):
            d_in = capi.DeviceBuffer(dev, table.nbytes)
            d_in.upload(table)
            capi.predict_device(model, d_in, rows, table.shape[1], d_out)
            out = d_out.download((rows, D * H))
            meds = []
            for _ in range(runs):
                ms = sorted(capi.time_predict_device(model, d_in, rows, table.shape[1], d_out, 3) / 3 for _ in range(REPS))
                meds.append(ms[len(ms) // 2])
            print(f"{name:<20} {label:<28} {rows} rows: " + " ".join(f"{m:8.3f}" for m in meds) + f" ms (n={runs} medians of {REPS}); "
                  f"median {sorted(meds)[len(meds) // 2]:8.3f}, spread {(max(meds) - min(meds)) / min(meds) * 100:4.1f} %", flush=True)
            return out

        capi.load_model(name, W.write(f"{d}/{name}.onnx", W.recurrent_from_spec(spec, flat=True, tail="y_h")))
        fixed = timed(name, x, "fixed length")
        capi.unload_model(name)
        if fixed_only:
            continue
        lname = name + "_lens"
        capi.load_model(lname, W.write(f"{d}/{lname}.onnx", W.recurrent_from_spec(spec, flat=True, tail="y_h", seq_lens=dict(form="rank1"))))
        for pattern in patterns:
            ln = lens_column(pattern, T, rows, rng)
            table = np.ascontiguousarray(np.concatenate([x, ln.reshape(-1, 1).astype(np.float32)], axis=1))
            out = timed(lname, table, f"lengths {pattern} (mean {ln.mean():.1f})")
            if pattern == "full":
                print(f"{name:<20} lengths full == fixed length, bit for bit: {np.array_equal(out.view(np.uint32), fixed.view(np.uint32))}", flush=True)
        capi.unload_model(lname)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lens", nargs="+", choices=["full", "quarter", "uniform", "uniform-sorted"])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--fixed-only", action="store_true")
    args = ap.parse_args()
    if args.lens or args.fixed_only:
        return lens_main(args.lens or [], args.runs, args.fixed_only)
    d = tempfile.mkdtemp()
    dev = capi.device_ordinal(0)
    for name, op, T, F, H, layers, direction, rows in SHAPES:
        spec = W.recurrent_spec(op, T=T, F=F, H=H, layers=layers, direction=direction)
        D = spec["D"]
        capi.load_model(name, W.write(f"{d}/{name}.onnx", W.recurrent_from_spec(spec, flat=True)))
        plan = capi.get_plan(name)["plan"]
        flop = plan["flops_per_row"]
        bytes_row = 4 * (T * F + T * D * H + 2 * (layers - 1) * T * D * H)
        rng = np.random.default_rng(1)
        for n in (rows, 2048):
            x = rng.normal(0, 1, (n, T * F)).astype(np.float32)
            d_in, d_out = capi.DeviceBuffer(dev, x.nbytes), capi.DeviceBuffer(dev, n * T * D * H * 4)
            d_in.upload(x)
            capi.predict_device(name, d_in, n, T * F, d_out)
            ms = [capi.time_predict_device(name, d_in, n, T * F, d_out, 3) / 3 for _ in range(REPS)]
            med = sorted(ms)[len(ms) // 2]
            rate = n / med * 1e3
            fp, fh = rate * flop / PEAK, rate * bytes_row / HBM
            print(f"{name:<20} device-resident {n:>8} rows: {spread(ms)} = {rate / 1e6:8.3f} M rows/s; {flop} flop/row -> {fp:5.3f} of the f32 MFMA peak; "
                  f"{bytes_row} B/row -> {fh:5.3f} of HBM; the nearer bound: {'matrix cores' if flop / PEAK > bytes_row / HBM else 'HBM'}", flush=True)
            del d_in, d_out
        host_rows = 2048 * 96
        xh = rng.normal(0, 1, (host_rows, T * F)).astype(np.float32)
        chunks = [xh[i:i + 2048] for i in range(0, host_rows, 2048)]
        rates = []
        for _ in range(3):
            nxt = [0]
            lock = threading.Lock()
            ready = threading.Barrier(17)

            def worker():
                capi.predict(name, chunks[0])  # this thread's stream, staging and scratch exist before the clock starts
                ready.wait()
                while True:
                    with lock:
                        i = nxt[0]
                        nxt[0] += 1
                    if i >= len(chunks):
                        return
                    capi.predict(name, chunks[i])

            th = [threading.Thread(target=worker) for _ in range(16)]
            for t in th:
                t.start()
            ready.wait()
            t0 = time.perf_counter()
            for t in th:
                t.join()
            rates.append(host_rows / (time.perf_counter() - t0) / 1e6)
        print(f"{name:<20} end to end, infera_predict, 16 callers x 2048-row chunks: {sorted(rates)[1]:7.3f} M rows/s (min {min(rates):.3f}, max {max(rates):.3f}, n=3)",
              flush=True)
        capi.unload_model(name)
        try:
            import torch
        except ImportError:
            continue
        torch.set_num_threads(16)
        kw = dict(input_size=F, hidden_size=H, num_layers=layers, bidirectional=D == 2, batch_first=True)
        m = getattr(torch.nn, op)(**kw)
        xt = torch.from_numpy(xh[:8192].reshape(-1, T, F))
        with torch.no_grad():
            m(xt)
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                m(xt)
                ts.append(time.perf_counter() - t0)
        print(f"{name:<20} torch-CPU float32, 16 threads, 8192 rows: {8192 / sorted(ts)[1] / 1e6:7.3f} M rows/s (median of 3)", flush=True)


if __name__ == "__main__":
    main()
