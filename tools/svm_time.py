"""Times the SVM kernels (hip/svm.hip) on three shapes: an RBF SVC (30 features, 4096 SVs, 3 classes, probabilities served), an RBF SVR
(128 features, 16384 SVs) and a binary POLY SVC (8 features, 512 SVs, label served).  Per shape: device-resident rows/s on a 20M-row
table (4M for the SVR) and its fraction of the matrix-core bound 157.3e12 / (2 F_pad n_SV + stage-2 MFMA flop) per row; then end to
end through infera_predict with 16 caller threads on 2048-row chunks.
usage (GPU box): python tools/svm_time.py            all of the above
                 python tools/svm_time.py --chunk    only 2048-row calls, for `rocprofv3 --kernel-trace --stats -- python ...`"""
import os
import sys
import tempfile
import threading
import time

import numpy as np

sys.path.insert(0, os.getcwd())
from infera_amd import capi, onnx_writer as W, synth  # noqa: E402

PEAK = 157.3e12  # f32 MFMA, vendor peak
SHAPES = [  # name, features, n_sv, kind, classes, kernel, probabilities, output, rows
    ("svc_rbf_3c_prob", 30, 4096, "classifier", 3, "RBF", True, "probabilities", 20_000_000),
    ("svr_rbf", 128, 16384, "regressor", 1, "RBF", False, "label", 4_000_000),
    ("svc_poly_binary", 8, 512, "classifier", 2, "POLY", False, "label", 20_000_000),
]


def bound_flop(F, n_sv, classes):
    """MFMA flop per row as the kernel issues them: stage 1 on F_pad, stage 2 on 32-row tiles when C - 1 > 8"""
    F_pad = (F + 7) // 8 * 8
    f = 2 * F_pad * n_sv
    if classes - 1 > 8:
        f += 2 * 32 * ((classes - 1 + 31) // 32) * n_sv
    return f


def main():
    chunk_only = "--chunk" in sys.argv
    d = tempfile.mkdtemp()
    dev = capi.device_ordinal(0)
    for name, F, n_sv, kind, C, kernel, prob, output, rows in SHAPES:
        sample = synth.table(42, 0, 20000, F)
        spec = W.svm_spec(features=F, n_sv=n_sv, kind=kind, classes=C, kernel=kernel, probabilities=prob, seed=n_sv + F)
        spec["support_vectors"] = sample[np.random.default_rng(1).integers(0, sample.shape[0], spec["n_sv"])]
        capi.load_model(name, W.write(f"{d}/{name}.onnx", W.svm_from_spec(spec, output=output)))
        plan = capi.get_plan(name)
        k = [s for s in plan["plan"]["steps"] if s["kind"] == "SvmKernel"][0]
        oc = 1 if len(plan["plan"]["output_shape"]) == 1 else plan["plan"]["output_shape"][1]
        if chunk_only:
            x = synth.table(7, 0, 2048, F)
            for _ in range(200):
                capi.predict(name, x)
            print(f"{name}: 200 calls of 2048 rows", flush=True)
            capi.unload_model(name)
            continue
        d_in, d_out = capi.DeviceBuffer(dev, rows * F * 4), capi.DeviceBuffer(dev, rows * oc * 4)
        capi.synth_fill(d_in, 42, 0, rows, F)
        capi.predict_device(name, d_in, rows, F, d_out)
        ms = capi.time_predict_device(name, d_in, rows, F, d_out, 5) / 5
        rate = rows / ms * 1e3
        bf = bound_flop(F, n_sv, C)
        print(f"{name:<16} {kernel} F={F} n_SV={n_sv} C={C} slices={k['slices']} output={k['output']}: resident {ms:8.2f} ms / {rows // 1_000_000}M rows = "
              f"{rate / 1e6:8.1f} M rows/s; matrix-core bound 157.3e12 / {bf} flop/row = {PEAK / bf / 1e6:8.1f} M rows/s -> "
              f"{rate * bf / PEAK:5.3f} of it ({rate * plan['plan']['flops_per_row'] / 1e12:6.1f} TFLOP/s algorithmic)", flush=True)
        del d_in, d_out
        host_rows = 2_000_000
        xh = synth.table(42, 0, host_rows, F)
        chunks = [xh[i:i + 2048] for i in range(0, host_rows, 2048)]
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
        dt = time.perf_counter() - t0
        print(f"{name:<16} end to end, infera_predict, 16 callers x 2048-row chunks: {host_rows / dt / 1e6:7.1f} M rows/s", flush=True)
        capi.unload_model(name)


if __name__ == "__main__":
    main()
