"""Times the Nearest step (hip/nearest.hip), device resident: KMeans labels over 30 columns x 8 and x 256 centroids, 128 x 1024 (label
and transform), and a k-NN search of 128-d rows against 65,536 references (k = 10) at 2,048 and at 1M rows.  Per shape: rows/s, the
fraction of the step's own roofline -- 2 F_pad M flop per row at the fp32 MFMA peak, plus the [N, M] write at the HBM rate when it is
served -- and the operator-by-operator plan of the same graph (INFERA_NEAREST=0).
usage (GPU box): python tools/nearest_time.py [--quick] [--big-rows N]
                 --quick: 8x smaller row counts, no large search; --big-rows: rows of the large search (default 1M: 1.7e16 flop a pass)"""
import os
import sys
import tempfile

sys.path.insert(0, os.getcwd())
from infera_amd import capi, onnx_writer as W  # noqa: E402

PEAK, HBM = 157.3e12, 6.3e12  # f32 MFMA flop/s and HBM bytes/s, vendor peaks
SHAPES = [  # name, F, M, graph, output, k, rows, compare with the generic plan
    ("kmeans_30x8_label", 30, 8, "kmeans", "label", 1, 16_000_000, True),
    ("kmeans_30x256_label", 30, 256, "kmeans", "label", 1, 16_000_000, True),
    ("kmeans_128x1024_label", 128, 1024, "kmeans", "label", 1, 4_000_000, True),
    ("kmeans_128x1024_transform", 128, 1024, "kmeans", "scores", 0, 1_000_000, True),
    ("knn_128x65536_k10_2048", 128, 65536, "knn", "indices", 10, 2048, True),
    ("knn_128x65536_k10_1M", 128, 65536, "knn", "indices", 10, 1_000_000, False),
]


def run(name, blob, d, rows, F, oc, dev, reps):
    capi.load_model(name, W.write(f"{d}/{name}.onnx", blob))
    try:
        d_in, d_out = capi.DeviceBuffer(dev, rows * F * 4), capi.DeviceBuffer(dev, rows * oc * 4)
        capi.synth_fill(d_in, 42, 0, rows, F)
        capi.predict_device(name, d_in, rows, F, d_out)
        ms = capi.time_predict_device(name, d_in, rows, F, d_out, reps) / reps
        kinds = [s["kind"] for s in capi.get_plan(name)["plan"]["steps"]]
        return ms, kinds
    finally:
        capi.unload_model(name)


def main():
    quick = "--quick" in sys.argv
    big = int(sys.argv[sys.argv.index("--big-rows") + 1]) if "--big-rows" in sys.argv else 1_000_000
    d = tempfile.mkdtemp()
    dev = capi.device_ordinal(0)
    for name, F, M, graph, output, k, rows, generic in SHAPES:
        if name.endswith("_1M"):
            rows = big
        if quick:
            if rows >= 1_000_000 and graph == "knn":
                continue
            rows = max(2048, rows // 8)
        spec = W.kmeans_spec(F, M, seed=F + M)
        blob = W.kmeans_from_spec(spec, "gemm", output) if graph == "kmeans" else W.knn_search_from_spec(spec, k, output, "gemm", "sqeuclidean")
        oc = M if output == "scores" else max(k, 1)
        reps = 20 if rows <= 4096 else 1 if name.endswith("_1M") else 3
        ms, kinds = run(name, blob, d, rows, F, oc, dev, reps)
        F_pad = (F + 7) // 8 * 8
        t_bound = rows * (2 * F_pad * M / PEAK + (4 * M / HBM if output == "scores" else 0))
        line = f"{name:<28} rows={rows:>9} {'+'.join(kinds)}: {ms:9.3f} ms  {rows / ms * 1e3 / 1e6:9.2f} M rows/s  roofline fraction {t_bound * 1e3 / ms:5.3f}"
        if generic:
            os.environ["INFERA_NEAREST"] = "0"
            try:
                gms, gk = run(name + "_generic", blob, d, rows, F, oc, dev, reps)
            finally:
                del os.environ["INFERA_NEAREST"]
            line += f"  | generic {'+'.join(gk)}: {gms:9.3f} ms  x{gms / ms:5.2f}"
        print(line, flush=True)


if __name__ == "__main__":
    main()
