#!/usr/bin/env python3
"""bench.py -- rows/sec through the infera_predict hot path on MI355X (BASELINE.json metric).

A "step" is ONE pass of the hot path over one batch of synthetic input: the whole 10M-row x
128-feature FLOAT table of BASELINE config C2 (3-layer MLP 128->256->64->1), already resident in
HBM when the timed region starts, pushed through the model that infera_load_model lowered.  With
--gpus N each rank owns its own 10M-row range of an (N x 10M)-row table (row-range sharding, weak
scaling, no data-path collective); value = all rows of all ranks / max-over-ranks time.

A plain run sets up, warms up, times --steps steps and prints the driver-contract fields (with --dump-outputs DIR it first writes
what the last step computed to DIR/*.npy).  With --full the JSON line also carries
  * `roofline`     -- the dominant kernel against the gfx950 peak that bounds it (HIP events on the launching stream);
  * `end_to_end`   -- the metric as SURVEY.md 8(d) defines it: rows/s through the SQL surface's `infera_predict`
                      (T worker threads x 2048-row chunks of a columnar table in HOST memory: gather -> pinned staging
                      -> H2D -> kernel -> D2H -> result vector), median of 5 scans after a warm-up, with the PCIe
                      fraction and the honest ratio to the CPU baseline.  It is never `value`;
  * `cpu_baseline` -- the oracle ("port") scanning the same host table with the reference's execution shape.

Launch: `python bench.py` (N=1) or
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
      --master-port P bench.py --gpus N --steps K --warmup W
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

# torch first: its bundled HIP runtime must be the one libinfera.so binds to (one runtime per process)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

FP32_MFMA_PEAK_TFLOPS = 157.3  # MI355X_MICROARCH.md "Peak FP32 (matrix)"
BF16_MFMA_PEAK_TFLOPS = 2500.0  # dense bf16 (the headline figure with 2:1 sparsity is never used)
HBM_PEAK_GBS = 8000.0
DUMP_LIMIT_BYTES = 64 << 20  # --dump-outputs: all ranks' files together


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", type=int, default=None, help="table rows per GPU (default: C2 10M for mlp, C4 50M for logreg)")
    ap.add_argument("--workload", default="mlp", choices=["mlp", "logreg", "resnet18"])
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-seconds", type=float, default=12.0, help="target CPU-baseline sample duration")
    ap.add_argument("--precision", default="default", choices=["default", "fp32"],
                    help="resnet18 workload: fp32 = the tiled convolutions on the exact-fp32 matrix instruction instead of the default "
                         "bf16 x three exact parts (DESIGN.md 3.3)")
    ap.add_argument("--no-other-workloads", action="store_true",
                    help="default run only: skip the short device-resident C4 / C5 measurements reported under other_workloads")
    ap.add_argument("--no-end-to-end", action="store_true", help="skip the host-path (PCIe-inclusive) scan")
    ap.add_argument("--e2e-threads", default="", help="worker-thread counts to sweep for the host path (default: from the CPU budget)")
    ap.add_argument("--e2e-reps", type=int, default=5)
    ap.add_argument("--e2e-numa", default="auto", choices=["auto", "off"],
                    help="auto: the host-path scan (and the CPU baseline) run on the CPUs of the GPU's NUMA node -- worker threads, "
                         "host table and pinned staging local to the GPU's root complex (+3-4 %% rows/s, +6-20 %% on the bare H2D ceiling)")
    ap.add_argument("--host-path", action="store_true",
                    help="single process, --gpus N device slots (INFERA_DEVICES=0..N-1, or N slots on --share-device): "
                         "measure ONLY the host path, the shape DuckDB runs the extension in (SURVEY 8e)")
    ap.add_argument("--share-device", type=int, default=None,
                    help="testing only: every rank uses this one HIP device (lets the N>1 control path run on a 1-GPU box)")
    ap.add_argument("--no-registered", action="store_true", help="skip the scan over the REGISTERED host table (the opt-in zero-copy path)")
    ap.add_argument("--detail", default=os.path.join(ROOT, "bench_detail.json"), help="where the full (uncompacted) result object is written")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also measure and check everything beyond the headline figure: the roofline of the dominant "
                         "kernel, the other BASELINE configs (default run), the host path end to end (staged and registered), the CPU "
                         "baselines and the NaN check of the output.  Off: the run sets up, warms up, times the steps and prints the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write what the last step computed (the output array a caller of the device-resident "
                         "path receives) as DIR/output.npy, float32, DIR/output_rank<r>.npy per rank when N > 1; an output over "
                         f"{DUMP_LIMIT_BYTES >> 20} MB in all is cut to a fixed, seeded sample of its rows")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if args.dump_outputs and args.host_path:
        ap.error("--dump-outputs writes the device-resident path's output; --host-path has none")
    return args


def cpu_budget() -> dict:
    """Host CPUs this process may really use: logical CPUs, affinity mask and the cgroup v2/v1 CPU quota (containers
    often expose 256 logical CPUs with a quota of a few dozen; threads beyond the quota are throttled)."""
    logical = os.cpu_count() or 1
    try:
        affinity = len(os.sched_getaffinity(0))
    except AttributeError:
        affinity = logical
    quota = None
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()
        quota = None if q == "max" else float(q) / float(per)
    except (OSError, ValueError):
        try:
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            quota = None if q <= 0 else q / per
        except (OSError, ValueError):
            pass
    usable = min(affinity, int(quota)) if quota and quota >= 1 else affinity
    return {"logical_cpus": logical, "affinity": affinity, "cgroup_quota_cpus": quota, "usable": max(1, usable)}


def host_fma_peak_gflops_per_cpu() -> dict:
    """fp32 FMA peak of one host core: 2 FMA pipes x SIMD lanes x 2 flop x max clock (the figure a GEMM's GFLOP/s per CPU is read against)."""
    flags, mhz, name = "", 0.0, ""
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("flags") and not flags:
                flags = line
            elif line.startswith("model name") and not name:
                name = line.split(":", 1)[1].strip()
        mhz = float(open("/sys/devices/system/cpu/cpu0/cpufreq/cpuinfo_max_freq").read()) / 1e3
    except (OSError, ValueError):
        pass
    if not mhz:
        try:
            mhz = max(float(line.split(":")[1]) for line in open("/proc/cpuinfo") if line.startswith("cpu MHz"))
        except (OSError, ValueError):
            mhz = 0.0
    lanes = 16 if " avx512f" in flags else 8
    return {"cpu_model": name, "simd": "avx512f" if lanes == 16 else "avx2", "max_mhz": mhz,
            "fma_peak_gflops_per_cpu": 2 * lanes * 2 * mhz / 1e3,
            "note": "2 FMA pipes x lanes x 2 flop x max boost clock: an upper bound (sustained AVX clocks are lower; an SMT sibling shares the pipes)"}


def torch_cpu_leg(table, rows: int, cols: int, budget: dict, dims, softmax: bool, flops_row: float, seconds: float) -> dict:
    """The CPU leg this repository did NOT write: PyTorch's CPU operators (oneDNN / MKL) on the same 2048-row
    chunks of the same host table -- T worker threads with ONE intra-op thread each, the shape the reference gets from DuckDB's
    workers around a single-threaded Tract run.  oracle/torch_ref.py; never part of the product."""
    from infera_amd import sqlharness
    from oracle import torch_ref

    rg, top = sqlharness.ROW_GROUP, budget["usable"]
    try:
        n0 = min(rows, max(rg, 2048 * top * 4 // rg * rg))
        sec0, _ = torch_ref.scan_table(table, n0, cols, rg, top, dims, softmax)
        n = min(rows, max(rg, int(n0 / sec0 * seconds) // rg * rg))
        sec, _ = torch_ref.scan_table(table, n, cols, rg, top, dims, softmax)
    except Exception as exc:  # the leg must never cost the line
        return {"error": f"{type(exc).__name__}: {exc}"}
    return {"value": n / sec, "unit": "rows/s", "cores": top, "threads": top, "cpus": top, "kind": "torch-cpu", "rows": n, "seconds": sec,
            "gflops_per_cpu": n / sec * flops_row / 1e9 / top, "torch": torch.__version__,
            "what": "torch CPU F.linear / relu chain, torch.set_num_threads(1), T Python worker threads x 2048-row chunks gathered from the same host table"}


def cpu_baseline(model_path: str, table, rows: int, cols: int, target_s: float, budget: dict, flops_row: float, best_s: float = 4.0,
                 torch_dims=None, torch_softmax: bool = False) -> dict:
    """The oracle ("port") timed on this box's host cores with the reference's execution shape: T threads, 2048-row
    chunks of the SAME materialised host table the GPU path scans, single-threaded graph per chunk.  Table generation is
    outside the timed region.  T = best of a short sweep up to the CPU budget (oversubscribing a cgroup
    quota slows the scan down).  Two legs: `value` = reference-shaped (per-cell boxed gather + plain GEMM
    loop) and `best_cpu` = tiled gather + register-blocked AVX-512 / AVX2 micro-kernel GEMM (bit-identical results: what a
    packed SIMD matmul such as Tract's does with the same arithmetic)."""
    from infera_amd import sqlharness
    from oracle import oracle

    m = oracle.Model(model_path)
    top = budget["usable"]
    cands = sorted({max(1, top // d) for d in (8, 4, 2, 1)} | ({min(budget["affinity"], top * 2)} if budget["cgroup_quota_cpus"] else set()))
    rg = sqlharness.ROW_GROUP

    def sample_rows(want):  # whole row groups (or the whole table) so the sample's layout is the table's layout
        return rows if want >= rows else max(rg, int(want) // rg * rg)

    def leg(boxed, seconds):
        sweep, best_t, best_rate = {}, 1, 0.0
        for t in cands:
            n = sample_rows(2048 * t * (3 if boxed == 1 else 12))
            sec, _ = oracle.bench_scan_table(m, table, n, cols, threads=t, boxed=boxed)
            sweep[str(t)] = n / sec
            if n / sec > best_rate:
                best_t, best_rate = t, n / sec
        n = sample_rows(best_rate * seconds)
        sec, _ = oracle.bench_scan_table(m, table, n, cols, threads=best_t, boxed=boxed)
        cpus = min(best_t, top)
        return {"value": n / sec, "cores": best_t, "threads": best_t, "cpus": cpus, "rows": n, "seconds": sec, "thread_sweep_rows_per_s": sweep,
                "gflops_per_cpu": n / sec * flops_row / 1e9 / cpus, "cpus_counted": cpus}

    ref = leg(1, target_s)
    best = leg(2, min(target_s, best_s))
    nf = sample_rows(ref["value"] * min(target_s, 3.0))
    sec_fast, _ = oracle.bench_scan_table(m, table, nf, cols, threads=ref["cores"], boxed=False)
    peak = host_fma_peak_gflops_per_cpu()
    tleg = torch_cpu_leg(table, rows, cols, budget, torch_dims, torch_softmax, flops_row, min(target_s, best_s)) if torch_dims else None
    best.update({"unit": "rows/s", "kind": "port",
                 "what": "oracle/infera_oracle.c orc_bench_scan_table(boxed=2): 8x8-tiled transposing gather + register-blocked 6x32 (AVX-512) / 6x16 (AVX2) "
                         "micro-kernel GEMM, one k-ordered fmaf chain per output element (bit-identical to the plain loop, tests/test_oracle_blocked_gemm.py); "
                         "the instruction schedule of a packed SIMD matmul -- the class Tract's kernels are in",
                 "frac_of_fma_peak": best["gflops_per_cpu"] / peak["fma_peak_gflops_per_cpu"] if peak["fma_peak_gflops_per_cpu"] else None})
    return {"value": ref["value"], "unit": "rows/s", "cores": ref["cores"], "threads": ref["threads"], "cpus": ref["cpus"], "kind": "port",
            "cores_note": "`cores` = `threads` = the worker threads used (the contract's field); `cpus` = the CPUs those threads can occupy at once = "
                          "min(threads, this box's cgroup quota / affinity): 32 threads on a 16-CPU quota use 16 CPUs",
            "sample": f"first {ref['rows']} rows of the {rows}-row x {cols}-col f32 host table in 2048-row chunks, "
                      f"oracle/infera_oracle.c orc_bench_scan_table: boxed per-cell gather (infera_extension.cpp:199-227 cost class) + "
                      f"single-threaded graph per chunk, {ref['seconds']:.2f} s wall, table generation excluded",
            "thread_sweep_rows_per_s": ref["thread_sweep_rows_per_s"], "gflops_per_cpu": ref["gflops_per_cpu"],
            "fast_gather_value": nf / sec_fast,
            "fast_gather_note": "same scan with a plain strided gather instead of the boxed one (the gather was never the cost)",
            "best_cpu": best, **({"torch_cpu": tleg} if tleg else {}), "host_cpu": peak,
            "cpu_budget": budget,
            "caveat": "Tract itself cannot be built or timed in this image (no Rust toolchain, crate not vendored): `value` is the "
                      "reference-SHAPED CPU restatement (naive GEMM loop), `best_cpu` the same arithmetic through a register-blocked SIMD "
                      "micro-kernel, `torch_cpu` PyTorch's own CPU operators; ratios to the CPU are quoted against the FASTEST of the three"}


def cpu_baseline_blobs(model_path: str, cols: int, budget: dict, seconds: float = 10.0, flops_row: float = 3628146688.0) -> dict:
    """Config C5's CPU baseline: the oracle with the reference's BLOB execution shape -- one inference per ROW (the reference
    makes one FFI call and one batch-1 Tract run per BLOB, infera_extension.cpp:303-326), T threads.  `best_cpu`: the same
    with the register-blocked GEMM under the im2col convolutions."""
    from oracle import oracle

    m = oracle.Model(model_path)
    t = budget["usable"]

    def leg(boxed, secs):
        sec1, _ = m.bench_scan(t, cols, seed=42, threads=t, chunk_rows=1, boxed=boxed)  # one image per thread: sizes the sample
        rows = int(max(t, min(4096, t * max(1.0, secs / max(sec1, 1e-3)))))
        sec, _ = m.bench_scan(rows, cols, seed=42, threads=t, chunk_rows=1, boxed=boxed)
        return rows, sec

    rows, sec = leg(0, seconds)
    brows, bsec = leg(2, min(seconds, 4.0))
    peak = host_fma_peak_gflops_per_cpu()
    gf = brows / bsec * flops_row / 1e9 / t
    tleg = None
    try:  # the leg this repository did not write: torch's CPU conv stack (oneDNN), T threads x 8-image calls, one intra-op thread each
        from infera_amd import synth
        from oracle import torch_ref

        hw = int(round((cols // 3) ** 0.5))
        imgs = synth.table(7, 0, 16, cols)
        s1, _ = torch_ref.scan_images(imgs, 8 * t, hw, t)
        n = int(max(8 * t, min(4096, 8 * t * max(1.0, min(seconds, 4.0) / max(s1, 1e-3))))) // 8 * 8
        s2, _ = torch_ref.scan_images(imgs, n, hw, t)
        tleg = {"value": n / s2, "unit": "rows/s (images/s)", "cores": t, "kind": "torch-cpu", "rows": n, "seconds": s2,
                "gflops_per_cpu": n / s2 * flops_row / 1e9 / t, "torch": torch.__version__,
                "what": "torch CPU conv stack (BatchNorm folded), torch.set_num_threads(1), T Python worker threads x 8-image calls"}
    except Exception as exc:
        tleg = {"error": f"{type(exc).__name__}: {exc}"}
    return {"value": rows / sec, "unit": "rows/s (images/s)", "cores": t, "kind": "port",
            "sample": f"{rows} images of {cols} f32, one inference per row (the reference's per-BLOB FFI shape), oracle/infera_oracle.c on {t} threads, "
                      f"{sec:.2f} s wall (image generation included: < 0.1 % of a 3.6 GFLOP inference)",
            "gflops_per_cpu": rows / sec * flops_row / 1e9 / t,
            "best_cpu": {"value": brows / bsec, "unit": "rows/s (images/s)", "cores": t, "kind": "port", "rows": brows, "seconds": bsec, "gflops_per_cpu": gf,
                         "frac_of_fma_peak": gf / peak["fma_peak_gflops_per_cpu"] if peak["fma_peak_gflops_per_cpu"] else None,
                         "what": "the same scan with the register-blocked AVX-512 / AVX2 micro-kernel GEMM under the oracle's im2col convolutions (bit-identical results)"},
            "torch_cpu": tleg, "host_cpu": peak, "cpu_budget": budget,
            "caveat": "Tract itself cannot be built or timed in this image: `value` is the reference-shaped CPU restatement, `best_cpu` the same "
                      "arithmetic through a register-blocked SIMD GEMM; ratios are quoted against the faster"}


PCIE_RAW_GBS = 64.0         # PCIe Gen5 x16, one direction, raw
PCIE_ACHIEVABLE_GBS = 55.0  # what large pinned hipMemcpyAsync transfers reach


def end_to_end_blobs(model: str, images, blob_bytes: int, out_cols: int, threads_arg: str, reps: int, budget: dict) -> dict:
    """The BLOB path end to end (config C5): T threads x 2048-row chunks of an image table in host memory through
    infera_sql_call('infera_predict_from_blob') -- one batched engine call per chunk, pipelined pinned staging, H2D, the
    conv net, D2H, LIST result.  Rows cycle over the images held in `images` (a 1M-row x 602 KB table does not fit)."""
    from infera_amd import capi, sqlharness

    nimg = images.nbytes // blob_bytes
    cands = [int(x) for x in threads_arg.split(",")] if threads_arg else [4, 8, 16]
    cands = [t for t in cands if t <= max(4, 2 * budget["usable"])] or [4]
    sqlharness.bench_blob_scan(model, images, blob_bytes, 2048, 1, 1)  # contexts, pinned staging, scratch
    sweep = {}
    for t in cands:
        rows = 2048 * max(t, 4)
        secs, _ = sqlharness.bench_blob_scan(model, images, blob_bytes, rows, t, 1)
        sweep[str(t)] = rows / secs[0]
    best_t = int(max(sweep, key=sweep.get))
    rows = 2048 * max(best_t, 4) * 2
    secs, checksum = sqlharness.bench_blob_scan(model, images, blob_bytes, rows, best_t, reps)
    med = sorted(secs)[len(secs) // 2]
    rate = rows / med
    h2d = rate * blob_bytes / 1e9
    return {"rows_per_s": rate, "unit": "rows/s (images/s)", "rows_per_scan": rows, "threads": best_t, "scan_seconds": secs,
            "median_scan_seconds": med, "checksum": checksum, "host_images": nimg,
            "entry": "infera_sql_call('infera_predict_from_blob') per 2048-row chunk (one infera_predict_from_blob_batch per chunk: "
                     "pipelined pinned staging -> hipMemcpyAsync H2D -> conv net -> D2H -> LIST result); rows cycle over the host images",
            "thread_sweep_rows_per_s": sweep, "pcie_h2d_gbs_per_gpu": h2d, "pcie_peak_gbs": PCIE_RAW_GBS,
            "frac_of_pcie": h2d / PCIE_RAW_GBS, "pcie_bound_rows_per_s_per_gpu": {"raw": PCIE_RAW_GBS * 1e9 / blob_bytes},
            "device_slots": capi.get_devices()["devices"]}


def bind_to_gpu_numa_node(numa_node: int) -> dict:
    """Restricts this process (and every thread it creates from now on) to the CPUs of `numa_node`."""
    try:
        text = open(f"/sys/devices/system/node/node{numa_node}/cpulist").read().strip()
        cpus = set()
        for part in text.split(","):
            a, _, b = part.partition("-")
            cpus.update(range(int(a), int(b or a) + 1))
        cpus &= os.sched_getaffinity(0)
        if not cpus:
            return {"bound": False, "why": "no CPU of that node in the affinity mask"}
        os.sched_setaffinity(0, cpus)
        return {"bound": True, "numa_node": numa_node, "cpus": text}
    except (OSError, ValueError, AttributeError) as exc:
        return {"bound": False, "why": f"{type(exc).__name__}: {exc}"}


def end_to_end(fn: str, model: str, table, rows: int, cols: int, out_cols: int, threads_arg: str, reps: int, budget: dict,
               world: int, barrier, max_over_ranks, sweep_full: bool = True, scan=None, probe_h2d: bool = True) -> dict:
    """rows/s through the SQL surface: wall time from the first chunk's gather to the last result
    element consumed; median of `reps` scans after one warm-up; thread count = best of a sweep.  With N ranks the sweep runs
    in lockstep (a barrier before every candidate, the slowest rank's time decides) over 1x / 2x / 3x the ranks' share of
    the CPU budget: callers SLEEP while their chunk is in flight (naps between event queries), so more threads than CPUs is how a
    CPU quota is used up.  Reports CPU time per chunk (getrusage over the whole process), which -- not wall time per thread --
    is what bounds N GPUs fed from one CPU quota."""
    from infera_amd import capi, sqlharness

    scan = scan or sqlharness.bench_scan_table  # (sqlharness.bench_scan_segments: the same scan over a table in DuckDB's segment shape)
    top = budget["usable"]
    if threads_arg:
        cands = [int(x) for x in threads_arg.split(",")]
    elif world > 1:
        share = max(2, top // world)
        cands = sorted({min(24, share), min(24, 2 * share), min(24, 3 * share)})
    elif sweep_full:
        cands = sorted({t for t in (4, 8, 12, 16, 24, 32, 48) if t <= max(8, 3 * top)})
    else:
        cands = [min(24, max(8, top))]
    scan(fn, model, table, min(rows, 60 * 2048 * 4), cols, cands[0], 1)  # contexts, pinned buffers, code objects
    sweep = {}
    if len(cands) > 1:
        sweep_rows = rows if world == 1 else min(rows, 6_000_000)
        for t in cands:
            barrier()
            secs, _ = scan(fn, model, table, sweep_rows, cols, t, 1)
            sweep[str(t)] = sweep_rows * world / max_over_ranks(secs[0])
        top_rate = max(sweep.values())  # (identical on every rank: the rates are max-reduced)
        best_t = min(int(t) for t, v in sweep.items() if v >= 0.98 * top_rate)  # fewest threads within 2 % of the best: less CPU per chunk
        # the CPU cost per chunk is quoted from the fewest threads within 5 % of the best when that is fewer: callers beyond the CPU quota
        # add scheduler time to every chunk (24 threads on 16 CPUs: 78 us against 63-68 at 12-16) that a node with more CPUs would not pay
        cost_t = min(int(t) for t, v in sweep.items() if v >= 0.95 * top_rate)
    else:
        best_t = cost_t = cands[0]
    # what BARE pinned H2D copies reach on this box (two in flight per thread, set-up outside the clock, after the NUMA binding and the scans'
    # warm-up; best of the pipeline's own shape and three larger ones).  Reported for reference, NOT as a ceiling: round 5 measured bare 1 MiB
    # copies at 35-48 GB/s and 8 MiB copies at 53-55 on boxes where the pipeline moves its 1 MiB chunks at 56 -- a kernel behind every copy keeps
    # the queues busier than a copy alone.  The fraction to read is frac_of_pcie (against the link's raw 64 GB/s).
    dev0 = capi.device_ordinal(0)
    chunk_bytes = 2048 * cols * 4
    h2d_measured = max(capi.h2d_probe(dev0, chunk_bytes, 256, max(2, min(16, best_t))), capi.h2d_probe(dev0, 8 << 20, 48, 2),
                       capi.h2d_probe(dev0, 8 << 20, 32, 4), capi.h2d_probe(dev0, 2 << 20, 96, 8)) if probe_h2d else None
    before = {d["slot"]: d["host_rows"] for d in capi.get_devices()["devices"]}
    barrier()
    t0 = time.perf_counter()
    (secs, checksum), phases = sqlharness.phase_breakdown(scan, fn, model, table, rows, cols, best_t, reps)
    barrier()
    wall = max_over_ranks(time.perf_counter() - t0)
    secs_sorted = sorted(secs)
    med = secs_sorted[len(secs_sorted) // 2]
    med = max_over_ranks(med)  # slowest rank's median scan
    rate = rows * world / med
    per_gpu = rate / world
    h2d = per_gpu * cols * 4 / 1e9
    d2h = per_gpu * out_cols * 4 / 1e9
    after = capi.get_devices()["devices"]
    cost_rate = None
    if cost_t < best_t:
        barrier()
        (secs_c, _), phases_c = sqlharness.phase_breakdown(scan, fn, model, table, rows, cols, cost_t, max(2, reps // 2))
        cost_rate = rows * world / max_over_ranks(sorted(secs_c)[len(secs_c) // 2])
        phases = dict(phases, **{k: phases_c[k] for k in ("cpu_us_per_chunk", "sys_us_per_chunk", "cpus_busy", "gather") if k in phases_c})
    cpu_us = max_over_ranks(phases.get("cpu_us_per_chunk", 0.0))
    rows_per_cpu_s = 2048.0 / cpu_us * 1e6 if cpu_us > 0 else None
    host = {"cpu_us_per_chunk": cpu_us, "of_which_system_us": phases.get("sys_us_per_chunk"), "cpus_busy_during_scan": phases.get("cpus_busy"),
            "rows_per_cpu_second": rows_per_cpu_s, "measured_at_threads": cost_t, "rows_per_s_at_those_threads": cost_rate or rate,
            "what": "process CPU time (getrusage: user + system, every thread incl. the HIP runtime's) per 2048-row chunk over the timed scans; "
                    "rows_per_cpu_second = 2048 / cpu_us_per_chunk -- the host-side capacity one CPU of the quota adds, whatever the link does"}
    # the SECOND bound of the 8-GPU model: what the host's memory system delivers to staging buffers -- the staged path's own gather
    # routine over the same table, nothing sent to a GPU, at the scan's caller count and at one thread per CPU of the quota (all ranks at once)
    host_copy = None
    if probe_h2d and isinstance(table, np.ndarray) and phases.get("gather", 0) > 1.0:  # (a staged scan: the registered scans gather nothing)
        try:
            host_copy = {}
            for label, t in (("at_callers", best_t), ("at_quota", max(1, top // world))):
                barrier()
                g = sqlharness.bench_gather_only(table, rows, cols, t, 3)
                sec = max_over_ranks(min(g["scan_seconds"]))
                host_copy[label] = {"threads_per_rank": t, "gb_per_s": rows * world * cols * 4 / sec / 1e9, "cpu_us_per_chunk": g["cpu_us_per_chunk"]}
            host["host_copy"] = host_copy
            host["host_copy_gbs_at_threads"] = host_copy["at_quota"]["gb_per_s"]
        except Exception as exc:
            host["host_copy"] = {"error": f"{type(exc).__name__}: {exc}"}
            host_copy = None
    if rows_per_cpu_s and world == 1:
        quota = budget["usable"]
        cap = quota * rows_per_cpu_s
        copy_cap = host_copy["at_quota"]["gb_per_s"] * 1e9 / (cols * 4) if host_copy else None  # rows/s the quota's CPUs can gather, link or no link
        p8 = min(8 * rate, cap, copy_cap) if copy_cap else min(8 * rate, cap)
        host.update({
            "cpu_quota_assumed": quota,
            "host_capacity_rows_per_s_on_quota": cap,
            "host_copy_capacity_rows_per_s_on_quota": copy_cap,
            "predicted_rows_per_s_at_8_gpus": p8,
            "predicted_scaling_at_8_gpus": p8 / rate,
            "binding_bound": "8 x the 1-GPU rate" if p8 == 8 * rate else "cpu time per chunk" if p8 == cap else "host copy rate",
            "bounds_in_gpus": {"cpu_time": cap / rate, "host_copy": copy_cap / rate if copy_cap else None},
            "cpus_needed_for_6x": 6 * rate / rows_per_cpu_s,
            "prediction_note": f"8 GPUs fed from THIS box's quota of {quota} CPUs: min(8 x the 1-GPU rate, quota x rows_per_cpu_second, what {quota} threads gather per second "
                               f"with no GPU behind them) -- a prediction from the measured CPU cost per chunk (the gather into pinned staging is "
                               f"{phases.get('gather', 0):.0f} us of it) and the measured host copy rate on the GPU's NUMA node, not a measurement; "
                               f">= 6x needs {6 * rate / rows_per_cpu_s:.1f} CPUs at this cost per chunk"})
    from infera_amd import shard

    # every rank's own account of the timed scans (control plane: a gather of a few numbers): which device served how many rows, and its checksum
    mine = {"rank": int(os.environ.get("RANK", "0")), "ordinal": after[0]["ordinal"], "rows_this_run": sum(d["host_rows"] - before.get(d["slot"], 0) for d in after),
            "checksum": checksum, "median_scan_seconds": sorted(secs)[len(secs) // 2]}
    per_rank = shard.gather_objects(mine) if world > 1 else [mine]
    return {"rows_per_s": rate, "unit": "rows/s", "rows_per_scan_per_rank": rows, "ranks": world, "threads_per_rank": best_t, "per_rank": per_rank,
            "callers_per_gpu": best_t, "rows_per_s_per_gpu": per_gpu, "host_read_gbs": rate * cols * 4 / 1e9,
            "scan_seconds": secs, "median_scan_seconds": med, "all_reps_wall_seconds": wall, "checksum": checksum,
            "entry": f"infera_sql_call('{fn}') per 2048-row chunk (columnar gather -> infera_predict_columns -> pinned staging -> "
                     f"hipMemcpyAsync H2D -> kernel -> D2H -> result vector) over a materialised columnar table in host memory",
            "thread_sweep_rows_per_s": sweep,
            "host_cpu_cost": host,
            "pcie_h2d_gbs_per_gpu": h2d, "pcie_d2h_gbs_per_gpu": d2h,
            "pcie_peak_gbs": PCIE_RAW_GBS, "pcie_achievable_gbs": PCIE_ACHIEVABLE_GBS,
            "frac_of_pcie": h2d / PCIE_RAW_GBS, "frac_of_pcie_achievable": h2d / PCIE_ACHIEVABLE_GBS,
            "bare_h2d_copy_gbs": h2d_measured,
            "bare_h2d_copy_note": "plain pinned hipMemcpyAsync H2D on this box, no model, two copies in flight per thread (infera_hip_h2d_probe: T x one chunk, 2 x 8 MiB, "
                                  "4 x 8 MiB, 8 x 2 MiB threads x size, best) -- for reference, not a ceiling of the pipelined path (see bench.py)",
            "us_per_chunk_per_thread": phases,
            "pcie_bound_rows_per_s_per_gpu": {"raw": PCIE_RAW_GBS * 1e9 / (cols * 4), "achievable": PCIE_ACHIEVABLE_GBS * 1e9 / (cols * 4)},
            "device_slots": [{"slot": d["slot"], "ordinal": d["ordinal"], "rows_this_run": d["host_rows"] - before.get(d["slot"], 0)} for d in after]}


def duckdb_blocks_scan(fn: str, model: str, rows: int, cols: int, out_cols: int, seed: int, budget: dict, world: int, barrier, max_over_ranks,
                       all_ok=lambda ok: ok) -> dict:
    """The registered scan on DuckDB's BLOCK LAYOUT (profiles/r06_duckdb_blocks.txt): the table as column segments in 256 KiB
    blocks (8-byte header, 65,534 values) from the extension's registering allocator (sqlharness.SegmentTable), the chunk per row group that
    straddles two segments staged.  Two allocation orders: `callers` = every block of the table allocated in a RANDOM order -- 128 unrelated
    addresses per chunk, the pulling kernel for every chunk: the conservative row, and the one the 8-GPU prediction of the opt-in path is read
    from; `in_order` = a row group's 128 column blocks allocated back to back (a table loaded by one thread): out of the allocator's arena they
    lie at one 256 KiB stride inside one registration, and the 2-D copy applies as on a contiguous table."""
    from infera_amd import sqlharness

    prev = os.environ.get("INFERA_ZERO_COPY_ALLOCATOR")
    os.environ["INFERA_ZERO_COPY_ALLOCATOR"] = "1"
    out = {"rows": rows, "block_bytes": 262144, "header_bytes": 8, "values_per_segment": 65534,
           "layout": "per (row group, column) two 256 KiB blocks from the extension's registering (arena) allocator; first segment's vectors 8 bytes past a "
                     "16-byte boundary; the chunk per row group that straddles two segments is staged",
           "callers": {}, "in_order": {}}
    try:
        for key, shuffled, counts in (("callers", True, (2, 4, 8) if world == 1 else (4, 8)), ("in_order", False, (4, 8) if world == 1 else (4,))):
            seg, why = None, ""
            try:
                seg = sqlharness.SegmentTable(rows, cols, seed, min(32, max(1, budget["usable"] // world)), shuffled=shuffled)
                if not seg.registering_allocator:
                    why = "the registering allocator was not installed"
            except Exception as exc:
                why = f"{type(exc).__name__}: {exc}"
            if not all_ok(seg is not None and not why):
                if seg is not None:
                    seg.close()
                return {"error": why or "a peer rank could not build its segment table"}
            try:
                out["blocks"], out["create_seconds"] = seg.blocks, seg.create_seconds
                for t in counts:
                    d = end_to_end(fn, model, seg, rows, cols, out_cols, str(t), 3, budget, world, barrier, max_over_ranks, scan=sqlharness.bench_scan_segments,
                                   probe_h2d=False)
                    out[key][str(t)] = {"rows_per_s": d["rows_per_s"], "cpu_us_per_chunk": d["host_cpu_cost"]["cpu_us_per_chunk"]}
                out["assembled_chunks_per_scan_set"] = seg.assembled_chunks
            finally:
                seg.close()
        if world == 1:  # 8 GPUs on this box's CPU quota, from the CONSERVATIVE row: the best caller count under both bounds (8 x the per-GPU rate; CPUs / CPU time per chunk)
            quota = budget["usable"]
            best = max(((min(8 * v["rows_per_s"], quota * 2048e6 / v["cpu_us_per_chunk"]), int(t)) for t, v in out["callers"].items() if v["cpu_us_per_chunk"] > 0),
                       default=(None, None))
            out["predicted_rows_per_s_at_8_gpus"], out["predicted_at_callers_per_gpu"] = best
    finally:
        if prev is None:
            os.environ.pop("INFERA_ZERO_COPY_ALLOCATOR", None)
        else:
            os.environ["INFERA_ZERO_COPY_ALLOCATOR"] = prev
    return out


def end_to_end_registered(fn: str, model: str, table, rows: int, cols: int, out_cols: int, reps: int, budget: dict, world: int, barrier,
                          max_over_ranks, threads_arg: str = "", all_ok=lambda ok: ok, seed: int = 42) -> dict:
    """The same scan with the host table REGISTERED once (infera_hip_register_host_memory -- an opt-in for an application that owns
    long-lived column storage or opens DuckDB with the extension's registering allocator; NOT the drop-in path and never the headline).
    Every chunk is fetched in place (round 5: at most three 2-D copies in flight per GPU -- the runtime runs them one at a time -- and the
    pulling kernel for the other chunks; the CPU neither gathers nor enqueues a linear copy).  `rows_per_s` = the best of the caller sweep,
    `few_callers` = 4 callers per rank, which is what 8 GPUs fed from one small CPU quota run like."""
    from infera_amd import capi

    t0 = time.perf_counter()
    try:
        capi.register_host_memory(table)  # (pins the whole table: may hit the box's locked-memory limit -- then NO rank runs this phase)
        registered, why = True, ""
    except Exception as exc:
        registered, why = False, f"{type(exc).__name__}: {exc}"
    reg_s = time.perf_counter() - t0
    if not all_ok(registered):
        if registered:
            capi.unregister_host_memory(table)
        return {"error": why or "a peer rank could not register its table"}
    try:
        before = capi.zero_copy_calls()
        top = budget["usable"]
        share = max(2, top // world)
        # (a caller of this path costs ~20-29 us of CPU per ~60-80 us chunk -- it sleeps most of the time -- so callers, not CPUs, are what a rank needs:
        #  with N ranks on one quota the sweep oversubscribes the rank's CPU share up to 8 callers per GPU, where one GPU's link is full)
        th = threads_arg or ",".join(str(t) for t in (sorted({min(8, 2 * share), min(8, 4 * share)}) if world > 1 else sorted({max(2, share // 4), max(2, share // 2), share})))
        e = end_to_end(fn, model, table, rows, cols, out_cols, th, reps, budget, world, barrier, max_over_ranks)
        served = capi.zero_copy_calls() - before
        few = 4
        f = end_to_end(fn, model, table, rows, cols, out_cols, str(few), max(2, reps - 1), budget, world, barrier, max_over_ranks)
    finally:
        capi.unregister_host_memory(table)
    for k in ("bare_h2d_copy_gbs", "bare_h2d_copy_note", "pcie_achievable_gbs", "frac_of_pcie_achievable", "all_reps_wall_seconds"):
        e.pop(k, None)
    e["entry"] = (f"infera_sql_call('{fn}') per 2048-row chunk over a host table registered with infera_hip_register_host_memory: "
                  "infera_predict_columns -> the GPU fetches the chunk's 128 column runs out of the table itself (up to 3 chunks per GPU at a time by ONE 2-D copy each, "
                  "the others -- and typed / scattered columns -- by the pulling kernel) -> model kernels -> result vector")
    e["register_seconds"] = reg_s
    e["zero_copy_calls"] = served
    fh = f["host_cpu_cost"]
    e["few_callers"] = {"threads_per_rank": few, "rows_per_s": f["rows_per_s"], "cpu_us_per_chunk": fh["cpu_us_per_chunk"],
                        "frac_of_pcie": f["frac_of_pcie"], **{k: fh[k] for k in ("predicted_rows_per_s_at_8_gpus", "predicted_scaling_at_8_gpus", "cpus_needed_for_6x") if k in fh}}
    e["what"] = ("OPT-IN zero-copy path (include/infera_hip.h), not the drop-in path: no CPU gather, no pinned staging, no linear H2D copy -- "
                 "a third of the staged path's CPU time per chunk, which is what bounds 8 GPUs on one CPU quota")
    e["table_shape"] = "ONE contiguous registered range (qualifies for 2-D copies: a numpy / Arrow table; NOT DuckDB's storage shape -- see duckdb_blocks)"
    try:
        e["duckdb_blocks"] = duckdb_blocks_scan(fn, model, rows if world == 1 else min(rows, 4_000_000), cols, out_cols, seed, budget, world, barrier,
                                                max_over_ranks, all_ok)
    except Exception as exc:
        e["duckdb_blocks"] = {"error": f"{type(exc).__name__}: {exc}"}
    return e


def traffic_for(workload: str, rows: int):
    """HBM bytes per launch from the committed PMC passes (tools/profile_bench.sh), when they match this workload and row count."""
    tpath = os.path.join(ROOT, "profiles", f"traffic_{workload}.json")
    if os.path.exists(tpath):
        tj = json.load(open(tpath))
        if tj.get("rows") == rows:
            return tj["traffic_bytes_per_launch"], f"profiles/{os.path.basename(tpath)} (rocprofv3 PMC: 2*FETCH_SIZE + WRITE_SIZE, {tj.get('round', '')})"
    return None, None


OTHER = {
    "logreg": dict(rows=50_000_000, cols=128, out_cols=10, bound="hbm", flops_row=2560.0, bytes_row=552.0, passes=20, sql_fn="infera_predict_array",
                   name="C4: logistic regression Gemm(128->10)+Softmax(axis=1), 50M-row x 128-col FLOAT table resident in HBM"),
    "resnet18": dict(rows=1024, cols=3 * 224 * 224, out_cols=1000, bound="mfma", flops_row=3628146688.0, bytes_row=606112.0, passes=5, sql_fn=None,
                     name="C5: ResNet-18 topology (random weights), 1024 BLOB[3x224x224] f32 images resident in HBM"),
}


def other_model_path(onnx_writer, tmp: str, which: str) -> str:
    path = os.path.join(tmp, f"{which}.onnx")
    if not os.path.exists(path):
        onnx_writer.write(path, onnx_writer.logreg_softmax(128, 10) if which == "logreg" else onnx_writer.resnet18(in_hw=224))
    return path


def best_cpu_value(cb: dict) -> float:
    """The fastest CPU leg of a cpu_baseline block: reference-shaped port, register-blocked port, torch-CPU."""
    return max(cb["value"], cb["best_cpu"]["value"], (cb.get("torch_cpu") or {}).get("value", 0.0))


def roofline_of(bound: str, six: bool, flops_row: float, bytes_row: float, rows: int, kernel_s: float):
    if bound == "mfma" and six:  # six bf16 MFMAs per fp32 product (three exact parts per operand): the dense bf16 peak / 6
        return flops_row * rows / kernel_s / 1e12, BF16_MFMA_PEAK_TFLOPS / 6.0, "TFLOP/s"
    if bound == "mfma":
        return flops_row * rows / kernel_s / 1e12, FP32_MFMA_PEAK_TFLOPS, "TFLOP/s"
    return bytes_row * rows / kernel_s / 1e9, HBM_PEAK_GBS, "GB/s"


def other_workload(capi, onnx_writer, tmp: str, dev: int, which: str, precision: str = "default") -> dict:
    """BASELINE configs C4 / C5 beside the headline, device-resident (2 warm + `passes` timed passes, HIP events on the
    launching stream): the same definitions as `value` / `roofline`, so that the driver's own run records them too."""
    w = OTHER[which]
    rows, cols, out_cols, bound, flops_row, bytes_row = w["rows"], w["cols"], w["out_cols"], w["bound"], w["flops_row"], w["bytes_row"]
    model = "bench_" + which + ("_" + precision if precision != "default" else "")
    if precision != "default":
        os.environ["INFERA_PRECISION"] = precision  # (the convolution mode is read when a model is scheduled)
    try:
        capi.load_model(model, other_model_path(onnx_writer, tmp, which))
    finally:
        if precision != "default":
            os.environ.pop("INFERA_PRECISION", None)
    try:
        d_in = capi.DeviceBuffer(dev, rows * cols * 4)
        d_out = capi.DeviceBuffer(dev, rows * out_cols * 4)
        capi.synth_fill(d_in, 42, 0, rows, cols)
        for _ in range(2):
            capi.predict_device(model, d_in, rows, cols, d_out, sync=False)
        capi.sync(dev)
        iters = w["passes"]
        kernel_s = capi.time_predict_device(model, d_in, rows, cols, d_out, iters) / 1e3 / iters
        y = d_out.download((2, out_cols))
        assert all(v == v for v in y.ravel().tolist()), "NaN in output"
        plan = capi.get_plan(model)
        del d_in, d_out
    finally:
        capi.unload_model(model)
    six = "bf16x6" in str(plan.get("conv_precision", ""))
    achieved, peak, unit = roofline_of(bound, six, flops_row, bytes_row, rows, kernel_s)
    traffic, traffic_source = (None, None) if (bound == "mfma" and not six) else traffic_for(which, rows)
    return {"workload": w["name"], "rows": rows, "rows_per_s": rows / kernel_s, "ms_per_pass": kernel_s * 1e3, "passes_timed": iters,
            "dtype": "bf16x6 (f32 operands as three exact bf16 parts, six MFMAs per product, f32 accumulate)" if six else "f32",
            **({"vs_fp32_mfma_peak": achieved / FP32_MFMA_PEAK_TFLOPS, "peak_is": "dense bf16 MFMA peak / 6"} if six else {}),
            "value_is": "device_resident",
            "kernel": plan.get("fused_kernel", ",".join(sorted(set(plan["exec"]) - {"skipped"}))),
            "roofline": {"bound": bound, "achieved": achieved, "peak": peak, "unit": unit, "frac": achieved / peak, "traffic": traffic,
                         "traffic_source": traffic_source, "algorithmic_bytes": bytes_row * rows,
                         "algorithmic_per_row": {"flop": flops_row, "bytes": bytes_row}}}


def other_workload_host(capi, onnx_writer, tmp: str, which: str, table, trows: int, budget: dict, threads: int, no_cpu: bool) -> dict:
    """The same two configs END TO END and beside their CPU baselines, short: C4 over the host table C2's scan used (first 10M
    rows, list output of 10, 3 scans); C5 through infera_predict_from_blob over 512 host images (2 scans); CPU legs ~2 s each."""
    w = OTHER[which]
    model = "bench_" + which
    path = other_model_path(onnx_writer, tmp, which)
    capi.load_model(model, path)
    out = {}
    try:
        if which == "logreg":
            e = end_to_end(w["sql_fn"], model, table, trows, w["cols"], w["out_cols"], str(threads), 3, budget, 1, lambda: None, lambda v: v, sweep_full=False)
            for k in ("bare_h2d_copy_gbs", "bare_h2d_copy_note", "pcie_achievable_gbs", "frac_of_pcie_achievable", "all_reps_wall_seconds"):
                e.pop(k, None)
            out["end_to_end"] = e
            if not no_cpu:
                out["cpu_baseline"] = cpu_baseline(path, table, trows, w["cols"], 2.0, budget, w["flops_row"], best_s=2.0, torch_dims=(128, 10), torch_softmax=True)
        else:
            from infera_amd import synth

            images = synth.table(7, 0, 512, w["cols"])  # 512 images = 308 MB of host BLOBs
            out["end_to_end"] = end_to_end_blobs(model, images, w["cols"] * 4, w["out_cols"], "16", 2, budget)
            del images
            if not no_cpu:
                out["cpu_baseline"] = cpu_baseline_blobs(path, w["cols"], budget, seconds=2.0, flops_row=w["flops_row"])
        if "cpu_baseline" in out:
            cb = out["cpu_baseline"]
            out["end_to_end"]["vs_cpu_baseline"] = out["end_to_end"]["rows_per_s"] / best_cpu_value(cb)
            out["end_to_end"]["vs_cpu_reference_shaped"] = out["end_to_end"]["rows_per_s"] / cb["value"]
    finally:
        capi.unload_model(model)
    return out


# ---- the ONE line the driver parses: contract fields + the numbers a reader needs, no prose (the 20.9 KB line of round 3
# ---- overflowed the driver's 8 KB stdout window and parsed as null).  Everything else goes to bench_detail.json and to stderr.
LINE_LIMIT = 4096
CONTRACT_FIELDS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "value_is")


def _r(v, sig: int = 5):
    if isinstance(v, float):
        return float(f"{v:.{sig}g}")
    return v


def _pick(d, keys, sig: int = 5):
    return {k: _r(d[k], sig) for k in keys if isinstance(d, dict) and d.get(k) is not None}


def compact_cpu(cb: dict) -> dict:
    out = _pick(cb, ("value", "unit", "cores", "threads", "cpus", "kind", "gflops_per_cpu"))
    if "sample" in cb:
        out["sample"] = cb["sample"].split(",")[0][:96]
    if "best_cpu" in cb:
        out["best_cpu"] = _pick(cb["best_cpu"], ("value", "threads", "cpus", "gflops_per_cpu", "frac_of_fma_peak"))
    if cb.get("torch_cpu"):
        out["torch_cpu"] = _pick(cb["torch_cpu"], ("value", "threads", "cpus", "gflops_per_cpu", "error"))
    if "cpu_budget" in cb:
        out["cpu_quota"] = cb["cpu_budget"].get("usable")
    return out


def compact_e2e(e: dict) -> dict:
    out = _pick(e, ("rows_per_s", "rows_per_s_per_gpu", "frac_of_pcie", "bare_h2d_copy_gbs", "host_read_gbs", "vs_cpu_baseline", "vs_cpu_reference_shaped", "zero_copy_calls",
                    "vs_staged", "predicted_8_gpus_vs_staged_1_gpu", "alone_rows_per_s", "scaling_vs_alone", "vs_staged_alone", "error"))
    if "threads_per_rank" in e or "threads" in e:
        out["threads"] = out["callers_per_gpu"] = e.get("threads_per_rank", e.get("threads"))
    h = e.get("host_cpu_cost") or {}
    out.update(_pick(h, ("cpu_us_per_chunk", "measured_at_threads", "predicted_scaling_at_8_gpus", "cpus_needed_for_6x", "host_copy_gbs_at_threads", "binding_bound")))
    if h.get("bounds_in_gpus"):
        out["bounds_in_gpus"] = {k: _r(v, 3) for k, v in h["bounds_in_gpus"].items() if v}
    if e.get("few_callers"):
        out["few_callers"] = _pick(e["few_callers"], ("threads_per_rank", "rows_per_s", "cpu_us_per_chunk", "predicted_scaling_at_8_gpus"))
    blk = e.get("duckdb_blocks")
    if isinstance(blk, dict):  # [M rows/s, CPU us per chunk] by callers per GPU, on DuckDB's block layout
        out["duckdb_blocks"] = ({"error": str(blk["error"])[:80]} if "error" in blk else
                                {**{t: [_r(v["rows_per_s"] / 1e6, 4), _r(v["cpu_us_per_chunk"], 3)] for t, v in blk.get("callers", {}).items()},
                                 "in_order": {t: [_r(v["rows_per_s"] / 1e6, 4), _r(v["cpu_us_per_chunk"], 3)] for t, v in blk.get("in_order", {}).items()},
                                 **({"vs_staged_alone": {t: _r(v, 3) for t, v in blk["vs_staged_alone"].items()}} if "vs_staged_alone" in blk else {})})
    if e.get("prediction_from"):
        out["prediction_from"] = e["prediction_from"].split(" ")[0]
    return out


def compact_line(full: dict) -> dict:
    line = {k: full[k] for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline")}
    line["value"], line["ms_per_step"] = _r(full["value"], 7), _r(full["ms_per_step"], 7)
    line["dtype"] = full["dtype"].split(" ")[0]
    line["data"] = "synthetic"
    c = full["config"]
    line["config"] = {"workload": c["workload"][:120],
                      **_pick(c, ("rows_per_gpu", "rows", "features", "parallelism", "precision", "INFERA_DEVICES")), "kernel": str(c.get("kernel", ""))[:64]}
    line["value_is"] = full["value_is"].split(" ")[0]
    if isinstance(full.get("end_to_end"), dict) and "rows_per_s" in full["end_to_end"]:
        # BASELINE.json's metric as SURVEY 8(d) defines it (host table in, result vector out), whole job, all ranks scanning at once -- beside
        # `value` at EVERY N: the scaling question (north_star: >= 6x at 8 GPUs) is answered by this field of the N = 1 and N = 8 lines
        line["value_end_to_end"] = _r(full["end_to_end"]["rows_per_s"], 7)
        if full.get("scaling_vs_alone"):
            line["value_end_to_end_alone"] = _r(full["value_end_to_end_alone"], 7)
            line["scaling_vs_alone"] = _r(full["scaling_vs_alone"], 4)
    if "roofline" in full:
        line["roofline"] = _pick(full["roofline"], ("bound", "achieved", "peak", "unit", "frac", "traffic", "algorithmic_bytes", "kernel_ms", "vs_fp32_mfma_peak"), 6)
        line["roofline"].setdefault("traffic", None)
    if "cpu_baseline" in full:
        line["cpu_baseline"] = compact_cpu(full["cpu_baseline"])
    if "end_to_end" in full:
        line["end_to_end"] = compact_e2e(full["end_to_end"])
    if "end_to_end_registered" in full:
        line["end_to_end_registered"] = compact_e2e(full["end_to_end_registered"])
    if full.get("other_workloads"):
        ow = {}
        for key, w in full["other_workloads"].items():
            if "error" in w:
                ow[key] = {"error": str(w["error"])[:80]}
                continue
            o = _pick(w, ("rows", "rows_per_s", "ms_per_pass", "speedup_over_fp32"))
            o["dtype"] = w["dtype"].split(" ")[0]
            o["roofline"] = _pick(w["roofline"], ("bound", "frac", "achieved", "peak", "unit", "traffic"))
            if "end_to_end" in w:
                o["end_to_end"] = _pick(w["end_to_end"], ("rows_per_s", "frac_of_pcie", "vs_cpu_baseline", "error"))
            if "cpu_baseline" in w:
                cb = w["cpu_baseline"]
                o["cpu"] = {"port": _r(cb["value"]), "best_port": _r(cb["best_cpu"]["value"]), "torch": _r((cb.get("torch_cpu") or {}).get("value"))}
            ow[key] = o
        line["other_workloads"] = ow
    line["detail"] = "bench_detail.json (also on stderr)"
    return line


_LINE_OUT = None  # the process's ORIGINAL stdout (claim_stdout): where the one JSON line goes


def claim_stdout() -> None:
    """Keeps the driver's stdout for the ONE JSON line: file descriptor 1 is pointed at stderr for everything else this process and the
    libraries in it print (gloo announces "[Gloo] Rank 0 is connected to 1 peer ranks" on stdout from C++, HIP runtime warnings, ...)."""
    global _LINE_OUT
    if _LINE_OUT is None:
        sys.stdout.flush()
        _LINE_OUT = os.fdopen(os.dup(1), "w")
        os.dup2(2, 1)


def emit(full: dict, detail_path: str) -> None:
    """Full object -> stderr + the detail file; the compact line (<= LINE_LIMIT bytes) -> stdout, last."""
    text = json.dumps(full)
    try:
        with open(detail_path, "w") as fh:
            fh.write(text + "\n")
    except OSError as exc:
        print(f"bench.py: could not write {detail_path}: {exc}", file=sys.stderr)
    print("BENCH_DETAIL " + text, file=sys.stderr, flush=True)
    line = json.dumps(compact_line(full), separators=(",", ":"))
    if len(line) > LINE_LIMIT:  # never again an unparseable line: drop the optional blocks, largest first, then everything but the contract
        c = compact_line(full)
        for k in ("other_workloads", "end_to_end_registered", "cpu_baseline", "end_to_end", "roofline"):
            c.pop(k, None)
            line = json.dumps(c, separators=(",", ":"))
            if len(line) <= LINE_LIMIT:
                break
        if len(line) > LINE_LIMIT:  # (cannot happen with the fields above; a hard stop all the same: valid JSON, contract fields only, strings cut)
            c = {k: (v[:60] if isinstance(v, str) else v) for k, v in c.items() if k in CONTRACT_FIELDS}
            c["config"] = {"workload": str(full["config"].get("workload", ""))[:60]}
            line = json.dumps(c, separators=(",", ":"))
    print(line, file=_LINE_OUT or sys.stdout, flush=True)


def dump_sample_rows(rows: int, out_cols: int, world: int):
    """The rows --dump-outputs keeps of a rows x out_cols float32 output: None (all of them) when they fit this rank's share of
    DUMP_LIMIT_BYTES, else a fixed sample (seed 0, ascending, no repeats) that does."""
    budget = DUMP_LIMIT_BYTES // world - 4096  # (room for the .npy header)
    if rows * out_cols * 4 <= budget:
        return None
    return np.unique(np.random.default_rng(0).integers(0, rows, size=budget // (out_cols * 4)))


def dump_outputs(d_out, rows: int, out_cols: int, out_dir: str, rank: int, world: int) -> str:
    """--dump-outputs: what the last timed step wrote (rows x out_cols float32, the array infera_hip_predict_device hands its caller) ->
    out_dir/output.npy (output_rank<r>.npy when N > 1).  Over this rank's share of DUMP_LIMIT_BYTES only a fixed sample of rows is kept
    (seed 0, ascending row order): the same rows on every run, so that two builds of the library compare output for output."""
    y = d_out.download((rows, out_cols))
    keep = dump_sample_rows(rows, out_cols, world)
    if keep is not None:
        y = y[keep]
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, ("output" if world == 1 else f"output_rank{rank}") + ".npy")
    np.save(path, y)
    print(f"bench.py: wrote {path} ({y.shape[0]} of {rows} rows x {out_cols})", file=sys.stderr, flush=True)
    return path


def relaunch_command(gpus: int, host_path: bool, argv: list, env: dict):
    """`python bench.py --gpus N` with N > 1 and NO launcher around it (the shape the driver uses at N = 1) is one process
    with no WORLD_SIZE: it used to scan one shard on GPU 0 and print "n_gpus": 1.  Returns the `torch.distributed.run` command that runs the
    N ranks the flag asks for (one per GPU, rendezvous on 127.0.0.1 at a free port) -- or None when this process is already a rank, when
    N = 1, or for --host-path (ONE process over N device slots by definition)."""
    if gpus <= 1 or host_path or "WORLD_SIZE" in env or "RANK" in env:
        return None
    import socket

    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(gpus), "--master-addr", "127.0.0.1",
            "--master-port", str(port), os.path.abspath(__file__)] + list(argv)


def main():
    args = parse_args()
    cmd = relaunch_command(args.gpus, args.host_path, sys.argv[1:], os.environ)
    if cmd:
        print(f"bench.py: --gpus {args.gpus} without a launcher: re-executing as {args.gpus} ranks under torch.distributed.run", file=sys.stderr, flush=True)
        os.execv(cmd[0], cmd)
    claim_stdout()
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus and not args.host_path:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if args.host_path and world > 1:
        raise SystemExit("--host-path is the single-process shape: run it without torch.distributed.run")
    dev = local_rank if args.share_device is None else args.share_device
    if args.host_path:
        # DuckDB's shape: ONE process, its worker threads dealt round-robin over N device slots
        slots = [str(i) for i in range(args.gpus)] if args.share_device is None else [str(args.share_device)] * args.gpus
        os.environ["INFERA_DEVICES"] = ",".join(slots)
    else:
        # One process per GPU: this rank's library instance must only create a context / upload weights on
        # ITS device (read once at library load, so set before importing the binding).
        os.environ.setdefault("INFERA_DEVICES", str(dev))
    if args.precision != "default":
        os.environ["INFERA_PRECISION"] = args.precision  # (the convolution mode is read when a model is scheduled)
    if world > 1:
        # control plane only (barrier + max-reduce of one float); the data path has no collective
        # (a rank that dies inside a collective phase must cost the others minutes, not the default half hour: the contract line is still printed)
        from datetime import timedelta

        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=timedelta(seconds=600))
    torch.cuda.set_device(dev)
    torch.cuda.init()

    from infera_amd import capi, onnx_writer, shard, sqlharness

    if capi.device_count() < 1:
        raise SystemExit("bench.py needs a GPU: " + capi.get_devices()["reason"])
    # N=8 is BASELINE config C3 (the same MLP, 100M rows over 8 GPUs = 12.5M rows per rank); every other N keeps
    # C2's 10M rows per GPU.  Throughput per GPU does not depend on which of the two it is (both are >> one launch's
    # fill/drain), so the driver's N=1..8 series stays a weak-scaling series.
    c3 = args.workload == "mlp" and args.gpus == 8 and args.rows is None
    rows = args.rows or (12_500_000 if c3 else {"mlp": 10_000_000, "logreg": 50_000_000, "resnet18": 1024}[args.workload])
    hw = int(os.environ.get("INFERA_BENCH_RESNET_HW", "224"))  # experiments only; C5 is 224
    cols = 3 * hw * hw if args.workload == "resnet18" else 128
    tmp = tempfile.mkdtemp(prefix="infera_bench_")
    torch_dims, torch_softmax = None, False
    if args.workload == "mlp":
        path = onnx_writer.write(os.path.join(tmp, "mlp.onnx"), onnx_writer.mlp((128, 256, 64, 1)))
        out_cols = 1
        wl_name = ("C3: 3-layer MLP 128->256->64->1, 100M-row x 128-col FLOAT table row-range sharded over 8 GPUs (12.5M rows per GPU)" if c3
                   else "C2: 3-layer MLP 128->256->64->1 (Gemm+Relu, Gemm+Relu, Gemm), 10M-row x 128-col FLOAT table")
        bound, flops_row, bytes_row, sql_fn = "mfma", 98432.0, 516.0, "infera_predict"
        torch_dims = (128, 256, 64, 1)
    elif args.workload == "resnet18":
        path = onnx_writer.write(os.path.join(tmp, "resnet18.onnx"), onnx_writer.resnet18(in_hw=hw))
        out_cols, wl_name = 1000, "C5: ResNet-18 topology (random weights), BLOB[3x224x224] f32 images resident in HBM"
        bound, flops_row, bytes_row, sql_fn = "mfma", 3628146688.0, 606112.0, None  # (BLOB path: tools/blob_scan_bench.py)
    else:
        path = onnx_writer.write(os.path.join(tmp, "logreg.onnx"), onnx_writer.logreg_softmax(128, 10))
        out_cols, wl_name = 10, "C4: logistic regression Gemm(128->10)+Softmax(axis=1), 50M-row x 128-col FLOAT table, list output of 10"
        bound, flops_row, bytes_row, sql_fn = "hbm", 2560.0, 552.0, "infera_predict_array"
        torch_dims, torch_softmax = (128, 10), True
    capi.load_model("bench", path)
    plan = capi.get_plan("bench")
    budget = cpu_budget()
    barrier = shard.barrier

    if args.host_path:
        e2e_rows = args.rows or 10_000_000 * args.gpus  # one table, scanned by one process over N slots
        table = sqlharness.synth_table(e2e_rows, cols, 42, min(32, budget["usable"]))
        e2e = end_to_end(sql_fn, "bench", table, e2e_rows, cols, out_cols, args.e2e_threads, args.e2e_reps, budget, 1, barrier, shard.max_over_ranks)
        full = {"metric": "rows/sec through infera_predict (host path: one process, worker threads dealt over the device slots)",
                "value": e2e["rows_per_s"], "unit": "rows/s", "n_gpus": args.gpus, "steps": args.e2e_reps, "warmup": 1,
                "ms_per_step": e2e["median_scan_seconds"] * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
                "value_is": "end_to_end",
                "dtype": "f32", "data": "synthetic (counter-based splitmix64 table, seed 42; random-init weights seed 1234)",
                "config": {"workload": wl_name, "rows": e2e_rows, "features": cols, "INFERA_DEVICES": os.environ["INFERA_DEVICES"],
                           "parallelism": f"chunks round-robin over {args.gpus} device slots, no collective"},
                "end_to_end": e2e}
        emit(full, args.detail)
        return

    d_in = capi.DeviceBuffer(dev, rows * cols * 4)
    d_out = capi.DeviceBuffer(dev, rows * out_cols * 4)
    row0, _ = shard.row_range(rank, world, rows)
    capi.synth_fill(d_in, 42, row0, rows, cols)  # this rank's row range of the global table

    def step():
        capi.predict_device("bench", d_in, rows, cols, d_out, sync=False)

    for _ in range(args.warmup):
        step()
    capi.sync(dev)

    barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    capi.sync(dev)
    torch.cuda.synchronize()
    barrier()
    elapsed = time.perf_counter() - t0
    elapsed = shard.max_over_ranks(elapsed)
    if args.dump_outputs:
        dump_outputs(d_out, rows, out_cols, args.dump_outputs, rank, world)
    bf16x6 = "bf16x6" in str(plan.get("conv_precision", ""))

    def headline() -> dict:
        return {
            "metric": "rows/sec through infera_predict (device-resident table scan; PCIe-inclusive rate in end_to_end)",
            "value": rows * world * args.steps / elapsed,
            "value_is": "device_resident -- the bench contract's definition (inputs in HBM when the timed region starts).  BASELINE.json's metric as "
                        "SURVEY.md 8(d) defines it (host table in, result vector out, PCIe included) is end_to_end.rows_per_s in this same line; "
                        "ratios to the CPU baseline are only ever taken from that one",
            "unit": "rows/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "bf16x6 (f32 operands cut exactly into three bf16 parts, six bf16 MFMAs per product, f32 accumulate: the default form of the stem "
                     "and the tiled convolutions; the head on the exact-f32 instruction)" if bf16x6 else "f32",
            "data": "synthetic (counter-based splitmix64 table, seed 42; random-init weights seed 1234)",
            "config": {"workload": wl_name, "rows_per_gpu": rows, "features": cols, "parallelism": f"row-range x{world}",
                       "precision": str(plan.get("conv_precision", plan.get("precision", "fp32"))).split(" ")[0],
                       "entry": "infera_hip_predict_device (inputs resident in HBM)",
                       "kernel": plan.get("fused_kernel", ",".join(sorted(set(plan["exec"]) - {"skipped"})))},
        }

    if not args.full:  # a plain run: the headline figure and nothing else (the end_to_end / roofline / CPU figures are --full's)
        if rank == 0:
            emit(headline(), args.detail)
        if world > 1:
            dist.destroy_process_group()
        return

    # roofline of the dominant kernel: HIP events on the launching stream around back-to-back launches
    iters = max(3, min(args.steps, 10))
    ms = capi.time_predict_device("bench", d_in, rows, cols, d_out, iters)
    kernel_s = ms / 1e3 / iters
    achieved, peak, unit = roofline_of(bound, bf16x6, flops_row, bytes_row, rows, kernel_s)

    # HBM traffic per launch: PMC counters cannot be read from inside this process; they are collected by
    # tools/profile_bench.sh (separate rocprofv3 --pmc passes of this same command) and committed as
    # profiles/traffic_<workload>.json.  Reported only when that file matches this workload, row count AND the kernel the
    # plan reports (tests/test_traffic_profiles.py guards the constant against a kernel change).
    traffic, traffic_source = (None, None) if (args.precision == "fp32" and args.workload == "resnet18") else traffic_for(args.workload, rows)

    # a cheap end-of-run sanity check so a silently wrong kernel cannot post a number
    y = d_out.download((4, out_cols))
    assert os.environ.get("INFERA_CONV_PROBE") or all(map(lambda v: v == v, y.ravel().tolist())), "NaN in output"
    del d_in, d_out

    # ---- the other two GPU configs of BASELINE.json, short and device-resident (default single-GPU run only) ----
    others = {}
    default_run = args.workload == "mlp" and world == 1 and not args.no_other_workloads and args.rows is None
    if default_run:
        for key, which, prec in (("C4", "logreg", "default"), ("C5", "resnet18", "default"), ("C5_fp32", "resnet18", "fp32")):
            try:
                others[key] = other_workload(capi, onnx_writer, tmp, dev, which, prec)
            except Exception as exc:  # never at the expense of the headline line
                others[key] = {"error": f"{type(exc).__name__}: {exc}"}
        if all("rows_per_s" in others.get(k, {}) for k in ("C5", "C5_fp32")):
            others["C5"]["speedup_over_fp32"] = others["C5"]["rows_per_s"] / others["C5_fp32"]["rows_per_s"]

    # ---- the metric as SURVEY 8(d) defines it: the host path, PCIe included (all ranks scan concurrently) ----
    e2e, table = None, None
    e2e_error = None
    alone, alone_reg = None, None  # (N > 1: rank 0's scan with every other rank idle)
    numa = {"bound": False, "why": "--e2e-numa off"}
    if args.e2e_numa == "auto" and (sql_fn and not args.no_end_to_end or not args.no_cpu_baseline):
        node = capi.get_devices()["devices"][0].get("numa_node", -1)
        numa = bind_to_gpu_numa_node(node) if node >= 0 else {"bound": False, "why": "GPU's NUMA node unknown"}
        budget = cpu_budget()
    if args.workload == "resnet18" and not args.no_end_to_end and world == 1:
        try:
            from infera_amd import synth

            images = synth.table(7, 0, 512, cols)  # 512 images = 308 MB of host BLOBs
            e2e = end_to_end_blobs("bench", images, cols * 4, out_cols, args.e2e_threads, max(1, min(args.e2e_reps, 3)), budget)
            e2e["resident_rows_per_s"] = rows * args.steps / elapsed
        except Exception as exc:
            e2e_error = f"{type(exc).__name__}: {exc}"
    # With N ranks every host-path phase is collective (barriers, max over ranks).  A phase starts only when EVERY rank is ready for it
    # (all_ok), and an exception inside one -- a peer died: the barrier times out -- ends the collective phases on this rank; the contract
    # fields above are reported either way.
    dist_broken = False

    def all_ok(local_ok: bool) -> bool:
        nonlocal dist_broken
        if world == 1 or dist_broken:
            return local_ok and not dist_broken
        try:
            return shard.max_over_ranks(0.0 if local_ok else 1.0) == 0.0
        except Exception:
            dist_broken = True
            return False

    if sql_fn and not args.no_end_to_end:
        e2e_rows = min(rows, 10_000_000) if args.workload != "mlp" else rows
        try:
            table = sqlharness.synth_table(e2e_rows, cols, 42 + rank, min(32, max(1, budget["usable"] // world)))
        except Exception as exc:
            table, e2e_error = None, f"host table: {type(exc).__name__}: {exc}"
        if not all_ok(table is not None):
            table, e2e_error = None, e2e_error or "a peer rank could not materialise its host table"
        else:
            if world > 1:
                # Rank 0 ALONE first, every other rank waiting at the barrier: the 1-GPU reference of `scaling_vs_alone` is
                # measured on THIS box in THIS run, with the whole CPU budget behind one GPU -- what a plain N = 1 run of this file measures.
                if rank == 0:
                    try:
                        alone = end_to_end(sql_fn, "bench", table, e2e_rows, cols, out_cols, args.e2e_threads, max(2, min(args.e2e_reps, 3)), budget, 1,
                                           lambda: None, lambda v: v, sweep_full=False)
                        if not args.no_registered:
                            alone_reg = end_to_end_registered(sql_fn, "bench", table, e2e_rows, cols, out_cols, 2, budget, 1, lambda: None, lambda v: v, seed=42 + rank)
                    except Exception as exc:  # (the alone phase must never cost the collective one: the barrier below is reached either way)
                        alone_reg = {"error": f"{type(exc).__name__}: {exc}"}
                try:
                    barrier()
                except Exception as exc:
                    dist_broken = True
                    e2e_error = f"alone phase: {type(exc).__name__}: {exc}"
            if all_ok(not dist_broken):
                try:
                    e2e = end_to_end(sql_fn, "bench", table, e2e_rows, cols, out_cols, args.e2e_threads, args.e2e_reps, budget, world, barrier,
                                     shard.max_over_ranks)
                except Exception as exc:
                    dist_broken = world > 1
                    e2e_error = f"{type(exc).__name__}: {exc}"

    # ---- the same scan over a REGISTERED table (zero-copy path): what the host side costs without the gather ----
    e2e_reg = None
    if sql_fn and table is not None and not args.no_end_to_end and not args.no_registered and all_ok(e2e is not None):
        try:
            e2e_reg = end_to_end_registered(sql_fn, "bench", table, min(rows, 10_000_000) if args.workload != "mlp" else rows, cols, out_cols,
                                            max(2, min(args.e2e_reps, 3)), budget, world, barrier, shard.max_over_ranks, all_ok=all_ok, seed=42 + rank)
        except Exception as exc:
            dist_broken = world > 1
            e2e_reg = {"error": f"{type(exc).__name__}: {exc}"}

    # ---- C4 / C5 end to end + their CPU baselines, short (default single-GPU run) ----
    if default_run and not args.no_end_to_end and table is not None and e2e:
        trows = min(rows, 10_000_000)
        for key, which in (("C4", "logreg"), ("C5", "resnet18")):
            if "error" in others.get(key, {}):
                continue
            try:
                others[key].update(other_workload_host(capi, onnx_writer, tmp, which, table, trows, budget, e2e["threads_per_rank"], args.no_cpu_baseline))
            except Exception as exc:
                others[key]["end_to_end"] = {"error": f"{type(exc).__name__}: {exc}"}

    if rank == 0:
        full = headline()
        full["roofline"] = {"bound": bound, "achieved": achieved, "peak": peak, "unit": unit, "frac": achieved / peak,
                            "traffic": traffic, "traffic_source": traffic_source, "algorithmic_bytes": bytes_row * rows,
                            "kernel_ms": kernel_s * 1e3, "rows_per_s": rows / kernel_s, "algorithmic_per_row": {"flop": flops_row, "bytes": bytes_row}}
        if bf16x6:
            full["roofline"]["peak_is"] = ("dense bf16 MFMA peak / 6 (six matrix instructions per fp32 product: three exact bf16 parts per operand, the three "
                                           "smallest partial products dropped); the stem + max-pool kernel runs in the same arithmetic, the 512 -> 1000 head on the exact-fp32 instruction")
            full["roofline"]["vs_fp32_mfma_peak"] = achieved / FP32_MFMA_PEAK_TFLOPS
        if others:
            full["other_workloads"] = others
        if e2e:
            e2e["numa_binding"] = numa
            full["end_to_end"] = e2e
            if alone and alone.get("rows_per_s"):
                # N > 1: `value` is N independent resident scans (N x by construction); THIS is the scaling figure -- all ranks' end-to-end rate over
                # rank 0's own end-to-end rate with the node to itself, same box, same run
                e2e["alone"] = {k: alone[k] for k in ("rows_per_s", "threads_per_rank", "median_scan_seconds", "frac_of_pcie", "thread_sweep_rows_per_s") if k in alone}
                e2e["alone"]["cpu_us_per_chunk"] = (alone.get("host_cpu_cost") or {}).get("cpu_us_per_chunk")
                e2e["alone"]["predicted_scaling_at_8_gpus"] = (alone.get("host_cpu_cost") or {}).get("predicted_scaling_at_8_gpus")
                e2e["alone_rows_per_s"] = alone["rows_per_s"]
                e2e["scaling_vs_alone"] = e2e["rows_per_s"] / alone["rows_per_s"]
                full["value_end_to_end_alone"] = alone["rows_per_s"]
                full["scaling_vs_alone"] = e2e["scaling_vs_alone"]
            if e2e_reg:
                if "rows_per_s" in e2e_reg and e2e.get("rows_per_s"):
                    # the registered scan beside the headline: this run's rate, and (1 GPU) what its CPU cost predicts for 8 GPUs on this quota,
                    # both as multiples of the STAGED 1-GPU rate -- the >= 6x of north_star is asked of the drop-in path's 1-GPU number
                    e2e_reg["vs_staged"] = e2e_reg["rows_per_s"] / e2e["rows_per_s"]
                    p8 = (e2e_reg.get("host_cpu_cost") or {}).get("predicted_rows_per_s_at_8_gpus")
                    blk = e2e_reg.get("duckdb_blocks") or {}
                    if p8 and world == 1:
                        e2e_reg["predicted_8_gpus_vs_staged_1_gpu_contiguous_table"] = p8 / e2e["rows_per_s"]
                        # the figure to quote: from DuckDB's block layout (every chunk the pulling kernel's), not from the contiguous table
                        e2e_reg["predicted_8_gpus_vs_staged_1_gpu"] = (blk["predicted_rows_per_s_at_8_gpus"] if blk.get("predicted_rows_per_s_at_8_gpus") else p8) / e2e["rows_per_s"]
                        e2e_reg["prediction_from"] = "duckdb_blocks" if blk.get("predicted_rows_per_s_at_8_gpus") else "contiguous registered table (duckdb_blocks failed)"
                    if world > 1 and alone and alone.get("rows_per_s") and blk.get("callers"):
                        blk["vs_staged_alone"] = {t: v["rows_per_s"] / alone["rows_per_s"] for t, v in blk["callers"].items()}
                    if alone_reg and alone_reg.get("rows_per_s"):
                        e2e_reg["alone_rows_per_s"] = alone_reg["rows_per_s"]
                        e2e_reg["scaling_vs_alone"] = e2e_reg["rows_per_s"] / alone_reg["rows_per_s"]
                    if alone and alone.get("rows_per_s"):  # the opt-in path at N GPUs over the DROP-IN path at one: north_star's >= 6x is asked of that 1-GPU number
                        e2e_reg["vs_staged_alone"] = e2e_reg["rows_per_s"] / alone["rows_per_s"]
                full["end_to_end_registered"] = e2e_reg
        elif e2e_error:
            full["end_to_end"] = {"error": e2e_error}
        if world == 1 and not args.no_cpu_baseline and args.workload == "resnet18":
            cb = cpu_baseline_blobs(path, cols, budget)
            full["cpu_baseline"] = cb
            if e2e:
                e2e["vs_cpu_baseline"] = e2e["rows_per_s"] / best_cpu_value(cb)
                e2e["vs_cpu_reference_shaped"] = e2e["rows_per_s"] / cb["value"]
        elif world == 1 and not args.no_cpu_baseline:
            if table is None:
                table = sqlharness.synth_table(min(rows, 10_000_000), cols, 42, min(32, budget["usable"]))
            trows = table.size // cols
            cb = cpu_baseline(path, table, trows, cols, args.cpu_seconds, budget, flops_row, torch_dims=torch_dims, torch_softmax=torch_softmax)
            full["cpu_baseline"] = cb
            if e2e and sql_fn:
                best = best_cpu_value(cb)
                e2e["vs_cpu_baseline"] = e2e["rows_per_s"] / best
                e2e["vs_cpu_reference_shaped"] = e2e["rows_per_s"] / cb["value"]
                e2e["pcie_cap_on_ratio"] = e2e["pcie_bound_rows_per_s_per_gpu"]["raw"] / best
        emit(full, args.detail)
    if world > 1 and not dist_broken:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
