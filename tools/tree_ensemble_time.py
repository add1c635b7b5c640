"""Times the tree-ensemble kernels (hip/trees.hip) on three shapes: XGBoost-like (100 trees, depth 6, 30 features, E = 1), large GBDT
(500 trees, depth 8, 128 features, E = 1) and forest-like (100 ragged trees of depth ~20, 30 features, 3 classes, label served).
Per shape: device-resident rows/s on a 20M-row table, node visits/s (mean internal nodes a row visits, counted by walking 20k
rows on the host) and input bytes/s; then end to end through infera_predict with 16 caller threads on 2048-row chunks.
usage (GPU box): python tools/tree_ensemble_time.py            all of the above
                 python tools/tree_ensemble_time.py --chunk    only 2048-row calls, for `rocprofv3 --kernel-trace --stats -- python ...`"""
import os
import sys
import tempfile
import threading
import time

import numpy as np

sys.path.insert(0, os.getcwd())
from infera_amd import capi, onnx_writer as W, synth  # noqa: E402

SHAPES = [  # name, trees, depth, ragged, features, kind
    ("xgboost_like", 100, 6, False, 30, "regressor"),
    ("large_gbdt", 500, 8, False, 128, "regressor"),
    ("forest_like", 100, 20, True, 30, "classifier"),
]


def visits_per_row(spec, x):
    """mean internal nodes visited per row, all trees (host walk of the spec)"""
    tid, nid = spec["nodes_treeids"], spec["nodes_nodeids"]
    index = {(t, n): i for i, (t, n) in enumerate(zip(tid, nid))}
    feat = np.asarray(spec["nodes_featureids"])
    vals = spec["nodes_values"]
    leaf = np.array([m == "LEAF" for m in spec["nodes_modes"]])
    tch = np.array([index.get((t, c), 0) for t, c in zip(tid, spec["nodes_truenodeids"])])
    fch = np.array([index.get((t, c), 0) for t, c in zip(tid, spec["nodes_falsenodeids"])])
    kids = set(tch[~leaf]) | set(fch[~leaf])
    roots = [i for i in range(len(tid)) if i not in kids]
    rows = np.arange(x.shape[0])
    total = 0
    for r in roots:  # all modes are BRANCH_LEQ here
        cur = np.full(x.shape[0], r)
        while True:
            act = ~leaf[cur]
            if not act.any():
                break
            total += int(act.sum())
            c = cur[act]
            cur[act] = np.where(x[rows[act], feat[c]] <= vals[c], tch[c], fch[c])
    return total / x.shape[0]


def main():
    chunk_only = "--chunk" in sys.argv
    d = tempfile.mkdtemp()
    dev = capi.device_ordinal(0)
    for name, trees, depth, ragged, F, kind in SHAPES:
        sample = synth.table(42, 0, 20000, F)
        spec = W.tree_ensemble_spec(features=F, trees=trees, depth=depth, ragged=ragged, kind=kind, thresholds=sample[:256], seed=trees + F)
        capi.load_model(name, W.write(f"{d}/{name}.onnx", W.tree_ensemble_from_spec(spec)))
        plan = capi.get_plan(name)
        walk = [s for s in plan["plan"]["steps"] if s["kind"] == "TreeEnsemble"][0]
        oc = 1
        if chunk_only:
            x = synth.table(7, 0, 2048, F)
            for _ in range(200):
                capi.predict(name, x)
            print(f"{name}: 200 calls of 2048 rows", flush=True)
            capi.unload_model(name)
            continue
        rows = 20_000_000
        d_in, d_out = capi.DeviceBuffer(dev, rows * F * 4), capi.DeviceBuffer(dev, rows * oc * 4)
        capi.synth_fill(d_in, 42, 0, rows, F)
        capi.predict_device(name, d_in, rows, F, d_out)
        ms = capi.time_predict_device(name, d_in, rows, F, d_out, 5) / 5
        vpr = visits_per_row(spec, sample)
        print(f"{name:<13} trees={trees} depth={walk['max_depth']} F={F} E={walk['E']} nodes={walk['nodes']} slices={walk['slices']} "
              f"output={walk['output']}: resident {ms:8.2f} ms / 20M rows = {rows / ms / 1e6:6.3f} G rows/s, "
              f"{vpr:.1f} node visits/row -> {rows * vpr / ms / 1e6:6.1f} G visits/s, {rows * 4 * (F + oc) / ms / 1e6:6.1f} GB/s (in+out)",
              flush=True)
        del d_in, d_out
        # end to end: 16 callers, infera_predict on 2048-row host chunks
        host_rows = 8_000_000
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
        print(f"{name:<13} end to end, infera_predict, 16 callers x 2048-row chunks: {host_rows / dt / 1e6:7.1f} M rows/s", flush=True)
        capi.unload_model(name)


if __name__ == "__main__":
    main()
