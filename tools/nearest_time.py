"""Times the Nearest step (hip/nearest.hip), device resident: KMeans labels over 30 columns x 8 and x 256 centroids, 128 x 1024 (label
and transform), and a k-NN search of 128-d rows against 65,536 references (k = 10) at 2,048 and at 1M rows.  Per shape: rows/s, the
fraction of the step's own roofline -- 2 F_pad M flop per row at the fp32 MFMA peak, plus the [N, M] write at the HBM rate when it is
served -- and the operator-by-operator plan of the same graph (INFERA_NEAREST=0).
The k-NN vote (VOTES): per case the classifier model (Nearest + NearestVote), the search model of the same spec in the same process
(Nearest + NearestReduce, `indices`: the difference is what the vote costs over what ships), the vote step's own bound -- the lists read
plus the output written at the HBM rate -- and, as an outside yardstick, torch float32 cdist + topk + one_hot-sum on the same tensors.
usage (GPU box): python tools/nearest_time.py [--quick] [--big-rows N] [--vote]
                 --quick: 8x smaller row counts, no large search; --big-rows: rows of the large search (default 1M: 1.7e16 flop a pass);
                 --vote: the k-NN vote cases only"""
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
VOTES = [  # name, F, M, k, C, rows
    ("vote_30x4096_k5_c3", 30, 4096, 5, 3, 262_144),
    ("vote_128x65536_k10_c10", 128, 65536, 10, 10, 16_384),
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


def torch_vote_ms(spec, y, C, k, rows, F, reps):
    """float32 cdist + topk + one_hot-sum + argmax on the device, the same reference set and synthetic rows; device events around `reps` passes"""
    import numpy as np
    import torch

    c = torch.from_numpy(spec["centers"]).cuda()
    yy = torch.from_numpy(np.asarray(y, np.int64)).cuda()
    x = torch.randn(rows, F, device="cuda")

    def once():
        idx = torch.cdist(x, c).topk(k, dim=1, largest=False).indices
        return torch.nn.functional.one_hot(yy[idx], C).sum(1).argmax(1)

    once()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        once()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def votes(d, dev, quick):
    import numpy as np

    for name, F, M, k, C, rows in VOTES:
        if quick:
            rows //= 8
        spec = W.kmeans_spec(F, M, seed=F + M)
        y = np.random.default_rng(F + M).integers(0, C, M)
        reps = 40  # (about half a second per timed window)
        res = {}
        for rnd in range(2):  # (the two models alternate: the spread shows beside the difference)
            for what, blob, oc in (("label", W.knn_classifier_from_spec(spec, y, list(range(C)), k), 1), ("search", W.knn_search_from_spec(spec, k, "indices"), k),
                                   ("proba", W.knn_classifier_from_spec(spec, y, list(range(C)), k, output="probabilities"), C)):
                ms, kinds = run(f"{name}_{what}{rnd}", blob, d, rows, F, oc, dev, reps)
                res.setdefault(what, []).append(ms)
                res[what + "_kinds"] = kinds
        capi.load_model(name + "_plan", W.write(f"{d}/{name}_plan.onnx", W.knn_classifier_from_spec(spec, y, list(range(C)), k)))
        S = capi.get_plan(name + "_plan")["plan"]["steps"][1]["slices"]
        capi.unload_model(name + "_plan")
        # per row: S lists of 16 (value, index) pairs read, oc floats written
        bound = {w: rows * (8 * 16 * S + 4 * oc) / HBM * 1e3 for w, oc in (("label", 1), ("proba", C))}
        for what in ("label", "proba", "search"):
            a = res[what]
            print(f"{name:<24} rows={rows:>8} {what:<7}{'+'.join(res[what + '_kinds']):<22}: {min(a):9.3f} ms (runs {', '.join(f'{v:.3f}' for v in a)})"
                  + (f"  vote - search = {min(a) - min(res['search']):+8.3f} ms; the vote step's byte bound {bound[what]:.4f} ms" if what != "search" else ""), flush=True)
        try:
            print(f"{name:<24} rows={rows:>8} torch float32 cdist+topk+one_hot-sum+argmax: {torch_vote_ms(spec, y, C, k, rows, F, 5):9.3f} ms", flush=True)
        except Exception as exc:  # (the yardstick is optional: say why it is missing)
            print(f"{name:<24} torch yardstick not measured: {type(exc).__name__}: {exc}", flush=True)


def main():
    try:  # (the yardstick of the vote cases: torch finds the GPU only when it is imported before the HIP runtime is first used)
        import torch  # noqa: F401
    except ImportError:
        pass
    quick = "--quick" in sys.argv
    big = int(sys.argv[sys.argv.index("--big-rows") + 1]) if "--big-rows" in sys.argv else 1_000_000
    d = tempfile.mkdtemp()
    dev = capi.device_ordinal(0)
    if "--vote" in sys.argv:
        return votes(d, dev, quick)
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
    votes(d, dev, quick)


if __name__ == "__main__":
    main()
