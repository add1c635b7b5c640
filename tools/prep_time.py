"""Times the preprocessing kernel (hip/prep.hip) on the reference ColumnTransformer shape: 16 input columns -- 6 numeric (Imputer + Scaler),
8 categorical one-hot encoded with 100 categories in all, 2 ordinal (LabelEncoder, 20 keys each) -- so F' = 108 and a row moves
(16 + 108) * 4 = 496 bytes.  Reports the Prep step's device-resident rows/s, GB/s and fraction of the ~6.3 TB/s achievable HBM read
rate (MI355X_MICROARCH.md); the same with the LabelEncoder columns removed; and the Prep step's share of a full pipeline (this prep +
100 trees of depth 6), resident and end to end through infera_predict with 16 caller threads on 2048-row chunks.
usage (GPU box): python tools/prep_time.py            all of the above
                 python tools/prep_time.py --chunk    only 2048-row calls, for `rocprofv3 --kernel-trace --stats -- python ...`"""
import os
import sys
import tempfile
import threading
import time

import numpy as np

sys.path.insert(0, os.getcwd())
from infera_amd import capi, onnx_writer as W  # noqa: E402

HBM = 6.3e12  # achievable HBM read rate, bytes/s
ROWS = 20_000_000


def table(spec, rows, seed):
    """category codes, ordinal keys with some misses, numeric values with NaN: what a DuckDB scan would hand over"""
    rng = np.random.default_rng(seed)
    x = rng.normal(0, 1, (rows, spec["features"])).astype(np.float32)
    g = spec["groups"]
    for cats, c in zip(spec["cats"], g["categorical"]):
        x[:, c] = rng.choice(np.asarray(cats + [99], np.float32), rows)
    for t, c in zip(spec["ordinal"], g["ordinal"]):
        x[:, c] = rng.choice(np.asarray(t["keys"] + [77], np.float32), rows)
    for c in g["numeric"]:
        x[rng.random(rows) < 0.05, c] = np.nan
    return x


def resident(name, spec, d_in, rows, out_cols):
    dev = capi.device_ordinal(0)
    d_out = capi.DeviceBuffer(dev, rows * out_cols * 4)
    capi.predict_device(name, d_in, rows, spec["features"], d_out)
    ms = capi.time_predict_device(name, d_in, rows, spec["features"], d_out, 5) / 5
    del d_out
    return ms


def end_to_end(name, xh):
    chunks = [xh[i:i + 2048] for i in range(0, xh.shape[0], 2048)]
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
    return xh.shape[0] / (time.perf_counter() - t0)


def main():
    chunk_only = "--chunk" in sys.argv
    d = tempfile.mkdtemp()
    dev = capi.device_ordinal(0)
    ref = W.prep_spec()
    no_le = W.prep_spec(ordinal=0)
    trees = W.tree_ensemble_spec(features=W.prep_width(ref), trees=100, depth=6, seed=3)
    models = [("prep_ref", ref, W.prep_from_spec(ref), W.prep_width(ref)),
              ("prep_no_labelencoder", no_le, W.prep_from_spec(no_le), W.prep_width(no_le)),
              ("prep_100_trees", ref, W.prep_from_spec(ref, head=W.tree_head(trees)), 1)]
    if chunk_only:
        for name, spec, blob, oc in models:
            capi.load_model(name, W.write(f"{d}/{name}.onnx", blob))
            x = table(spec, 2048, 7)
            for _ in range(200):
                capi.predict(name, x)
            print(f"{name}: 200 calls of 2048 rows", flush=True)
            capi.unload_model(name)
        return
    res = {}
    for name, spec, blob, oc in models:
        capi.load_model(name, W.write(f"{d}/{name}.onnx", blob))
        plan = capi.get_plan(name)
        p = [s for s in plan["plan"]["steps"] if s["kind"] == "Prep"][0]
        x = table(spec, 1_000_000, 42)
        d_in = capi.DeviceBuffer(dev, ROWS * spec["features"] * 4)
        d_in.upload(np.tile(x, (ROWS // x.shape[0], 1)))  # (the 1M-row sample repeated: a 20M-row table)
        ms = resident(name, spec, d_in, ROWS, oc)
        rate = ROWS / ms * 1e3
        res[name] = ms
        bpr = (p["F_in"] + (p["F"] if oc > 1 else 0)) * 4
        line = (f"{name:<22} F_in={p['F_in']} F'={p['F']} onehot={p['onehot_cols']} lookup={p['lookup_cols']} R={p['rows_per_tile']}: resident "
                f"{ms:8.2f} ms / {ROWS // 1_000_000}M rows = {rate / 1e6:8.1f} M rows/s")
        if oc > 1:
            line += f"; {bpr} B/row -> {rate * bpr / 1e9:7.1f} GB/s = {rate * bpr / HBM:5.3f} of 6.3 TB/s"
        print(line, flush=True)
        del d_in
        if name == "prep_100_trees":
            print(f"{'':<22} the Prep step's share of the resident pipeline: {res['prep_ref'] / ms:5.3f} "
                  f"(prep alone {res['prep_ref']:.2f} ms, pipeline {ms:.2f} ms)", flush=True)
            for nm in ("prep_ref", name):
                r = end_to_end(nm, table(spec, 2_000_000, 43))
                print(f"{nm:<22} end to end, infera_predict, 16 callers x 2048-row chunks: {r / 1e6:7.1f} M rows/s", flush=True)
    for name, *_ in models:
        capi.unload_model(name)


if __name__ == "__main__":
    main()
