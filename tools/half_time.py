"""Times float16 networks (HDense, hip/hdense.hip) beside the same networks in f32 through the existing kernels, in one process: C2's
shape 128 -> 256 -> 64 -> 1, the tabular 30 -> 100 -> 2, and one 561-column layer (561 -> 64).  Each half network runs in both edge forms
(halves between the layers; INFERA_HDENSE_HALF=0: f32) and on the float path (INFERA_HDENSE=0: Dense + RoundHalf).  The graph input and
output stay f32 (Cast -> ... -> Cast), so a call streams 4 (K + M_last) bytes per row: reports device-resident rows/s, the achieved
fraction of the ~6.3 TB/s HBM read rate (MI355X_MICROARCH.md) and the ratio to the f32 model.
usage (GPU box): python tools/half_time.py"""
import os
import sys
import tempfile

sys.path.insert(0, os.getcwd())
from infera_amd import capi, onnx_writer as W  # noqa: E402

HBM = 6.3e12
SHAPES = [((128, 256, 64, 1), 4_000_000), ((30, 100, 2), 8_000_000), ((561, 64), 1_000_000)]


def resident(name, d_in, rows, cols, out_cols):
    d_out = capi.DeviceBuffer(capi.device_ordinal(0), rows * out_cols * 4)
    capi.predict_device(name, d_in, rows, cols, d_out)
    ms = capi.time_predict_device(name, d_in, rows, cols, d_out, 10) / 10
    del d_out
    return ms


def load_with(name, path, **env):
    os.environ.update(env)
    try:
        capi.load_model(name, path)
    finally:
        for k in env:
            del os.environ[k]


def main():
    d = tempfile.mkdtemp()
    dev = capi.device_ordinal(0)
    for dims, rows in SHAPES:
        tag = "x".join(map(str, dims))
        hpath = W.write(f"{d}/h_{tag}.onnx", W.half_from_spec(W.half_mlp_spec(dims, act="Relu")))
        fpath = W.write(f"{d}/f_{tag}.onnx", W.mlp(dims))
        capi.load_model("h_half", hpath)
        load_with("h_f32edge", hpath, INFERA_HDENSE_HALF="0")
        load_with("h_floatpath", hpath, INFERA_HDENSE="0")
        capi.load_model("f32", fpath)
        d_in = capi.DeviceBuffer(dev, rows * dims[0] * 4)
        capi.synth_fill(d_in, 42, 0, rows, dims[0])
        bpr = 4 * (dims[0] + dims[-1])
        names = ("f32", "h_floatpath", "h_f32edge", "h_half")
        ms = {n: resident(n, d_in, rows, dims[0], dims[-1]) for n in names}
        for n in names:
            rate = rows / ms[n] * 1e3
            print(f"{tag:<14} {n:<11} {ms[n]:8.3f} ms / {rows // 1_000_000}M rows = {rate / 1e6:8.1f} M rows/s; {bpr} B/row -> {rate * bpr / 1e9:7.1f} GB/s = "
                  f"{rate * bpr / HBM:5.3f} of 6.3 TB/s; x{ms['f32'] / ms[n]:5.2f} of the f32 model's rate   exec={capi.get_plan(n)['exec']}", flush=True)
        del d_in
        for n in names:
            capi.unload_model(n)


if __name__ == "__main__":
    main()
