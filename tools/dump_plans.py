#!/usr/bin/env python3
"""What a build of the library makes of every ONNX file under a directory: its plan, or the text of its refusal.

    python tools/dump_plans.py MODELS_DIR [LIBINFERA_SO] > plans.jsonl

One JSON line per `.onnx` file, sorted by path: {"path": <relative path>, "plan": <infera_hip_get_plan's result>} or
{"path": ..., "error": <the load error's full text>}.  Lowering needs no GPU, so this runs wherever the CPU suite does.  A process
loads ONE library (the second argument; default: the tree's own build): to compare two builds -- the check that a change to the
lowering (csrc/host/lowering.cpp, lower_*.cpp) leaves every plan and every refusal as it was -- run it once per library over the same
directory and `diff` the two outputs.  `pytest -m "not gpu" --basetemp=DIR` leaves the models the CPU suite writes under DIR (where a
test writes several models to one path, the last of them).
"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main(argv):
    if len(argv) not in (2, 3):
        sys.exit(__doc__)
    root = argv[1]
    from infera_amd import capi

    capi.load_library(os.path.abspath(argv[2]) if len(argv) == 3 else None)
    paths = sorted(os.path.relpath(os.path.join(d, f), root) for d, _, files in os.walk(root) for f in files if f.endswith(".onnx"))
    plans = 0
    for rel in paths:
        line = {"path": rel}
        try:
            capi.load_model("m", os.path.join(root, rel))
        except capi.InferaError as e:
            line["error"] = str(e)
        else:
            try:
                line["plan"] = capi.get_plan("m")  # (a failure here is a bug, not a refusal: it ends the run)
            finally:
                capi.unload_model("m")
            plans += 1
        print(json.dumps(line, sort_keys=True))
    print(f"{len(paths)} models: {plans} plans, {len(paths) - plans} refusals", file=sys.stderr)


if __name__ == "__main__":
    main(sys.argv)
