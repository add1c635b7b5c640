#!/usr/bin/env python3
"""Where the waves of mlp3_split_kernel are while it runs (build with `make PROBES=1`, load with INFERA_LIB_PATH).

In the probe build every wave of the kernel stamps s_memrealtime (100 MHz) after the LDS fill and at its exit and writes
[workgroup, wave, XCD, hardware id], entry, exit, tiles to a side buffer: one lane per wave, once per launch.  This tool runs
warm launches at --rows rows and prints, per kernel variant (INFERA_MLP3_VARIANT: 8 = tiles in fixed shares, 14 = tile queue),
the waves' residency as a fraction of the launch's span (first entry to last exit) by wave index, by CU and by XCD, the
tiles they took, and the spread of their finish times.

usage: python tools/mlp_wave_residency.py [--variants 8,14] [--launches 5] [--rows 10000000]
"""
import argparse
import ctypes as C
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from infera_amd import capi, onnx_writer  # noqa: E402


def pct(a, qs=(0, 10, 50, 90, 100)):
    return " ".join(f"{v:7.4f}" for v in np.percentile(a, qs))


def report(v, launches):
    """launches: list of [waves, 4] uint64 arrays."""
    print(f"== variant {v}: {len(launches)} warm launches, {launches[0].shape[0]} waves each")
    res_all, fin_all, tiles_all, span_us = [], [], [], []
    for p in launches:
        t0, t1 = p[:, 1].astype(np.int64), p[:, 2].astype(np.int64)
        start, span = t0.min(), float(t1.max() - t0.min())
        span_us.append(span / 100.0)
        res_all.append((t1 - t0) / span)
        fin_all.append((t1 - start) / span)
        tiles_all.append(p[:, 3].astype(np.int64))
    ident = launches[-1][:, 0]
    wave = ((ident >> np.uint64(20)) & np.uint64(15)).astype(int)
    res, fin, tiles = np.mean(res_all, axis=0), np.mean(fin_all, axis=0), np.mean(tiles_all, axis=0)
    print(f"span_us (first entry .. last exit): {' '.join(f'{s:.1f}' for s in span_us)}")
    print(f"entry skew: last entry at {np.mean([(p[:, 1].astype(np.int64).max() - p[:, 1].astype(np.int64).min()) / 100.0 for p in launches]):.1f} us after the first")
    print(f"residency, all waves: mean {res.mean():.4f}   percentiles 0/10/50/90/100: {pct(res)}")
    for lo, hi in ((0, 3), (4, 7)):
        m = (wave >= lo) & (wave <= hi)
        print(f"  waves {lo}-{hi}: residency mean {res[m].mean():.4f} min {res[m].min():.4f} | finish mean {fin[m].mean():.4f} | tiles mean {tiles[m].mean():.2f} min {tiles[m].min():.0f} max {tiles[m].max():.0f}")
    for w in range(8):
        m = wave == w
        print(f"    wave {w}: residency {res[m].mean():.4f}  finish {fin[m].mean():.4f}  tiles {tiles[m].mean():.2f}")
    # placement is per launch (a workgroup need not land on the same CU twice): group inside each launch, then pool
    cu_res, xcd_res, xcd_tiles = [], {}, {}
    for p, r, t in zip(launches, res_all, tiles_all):
        xcd = ((p[:, 0] >> np.uint64(24)) & np.uint64(15)).astype(int)
        hw = ((p[:, 0] >> np.uint64(32)) & np.uint64(0xFFFF)).astype(int)
        cu = xcd * 65536 + (hw & 0xFF00)  # XCD, shader engine, shader array, CU
        for c in np.unique(cu):
            cu_res.append(r[cu == c].mean())
        for x in np.unique(xcd):
            xcd_res.setdefault(x, []).append(r[xcd == x].mean())
            xcd_tiles.setdefault(x, []).append(t[xcd == x].sum())
    print(f"by CU ({len(cu_res) // len(launches)} per launch): residency percentiles 0/10/50/90/100: {pct(np.array(cu_res))}")
    print("by XCD: " + "  ".join(f"{x}: {np.mean(r):.4f} ({np.mean(xcd_tiles[x]):.0f} tiles)" for x, r in sorted(xcd_res.items())))
    print(f"finish times / span, percentiles 0/10/50/90/100: {pct(fin)}")
    print(f"tiles per wave: min {tiles.min():.0f} median {np.median(tiles):.0f} max {tiles.max():.0f}")
    return res.mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", default="8,14")
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--rows", type=int, default=10_000_000)
    a = ap.parse_args()
    lib = capi.load_library()
    if not hasattr(lib, "infera_hip_mlp3_probe_buffer"):
        sys.exit("this library has no probes: build with `make PROBES=1` and point INFERA_LIB_PATH at it")
    lib.infera_hip_mlp3_probe_buffer.argtypes = [C.c_void_p]
    lib.infera_hip_mlp3_probe_buffer.restype = None
    tmp = tempfile.mkdtemp()
    capi.load_model("res", onnx_writer.write(os.path.join(tmp, "mlp.onnx"), onnx_writer.mlp()))
    dev = capi.device_ordinal(0)
    waves = 8 * int(capi.get_devices()["devices"][0]["cus"])
    rows = a.rows
    d_in = capi.DeviceBuffer(dev, rows * 128 * 4)
    d_out = capi.DeviceBuffer(dev, rows * 4)
    d_probe = capi.DeviceBuffer(dev, waves * 32)
    capi.synth_fill(d_in, 42, 0, rows, 128)
    for v in [int(x) for x in a.variants.split(",")]:
        os.environ["INFERA_MLP3_VARIANT"] = str(v)
        lib.infera_hip_mlp3_probe_buffer(None)
        for _ in range(3):  # warm
            capi.predict_device("res", d_in, rows, 128, d_out)
        lib.infera_hip_mlp3_probe_buffer(C.c_void_p(d_probe.ptr))
        launches = []
        for _ in range(a.launches):
            d_probe.upload(np.zeros((waves, 4), np.uint64))
            capi.predict_device("res", d_in, rows, 128, d_out)
            launches.append(d_probe.download((waves, 4), np.uint64))
        lib.infera_hip_mlp3_probe_buffer(None)
        report(v, launches)


if __name__ == "__main__":
    main()
