"""Times the Spectrum step (hip/spectrum.hip) device-resident and warm: STFT -> power of ROWS signals of L samples at n = 256, hop = 64 and
n = 1024, hop = 256, the centred (reflect Pad absorbed) mixed-radix n = 400, hop = 160 and, beside it, n = 512, hop = 160 un-centred (what
a user of 400-sample frames had to settle for before, on another bin grid); frames-major and bins-before-frames.
  (1) the step's time (HIP events around 3 back-to-back calls after a warm call, median of REPS windows) and its rate in TB/s of the bytes
      it reads plus writes (4 (L + frames bins) per signal);
  (2) in the same process, a plain elementwise pass of this project (Relu) over buffers of the size of the step's OUTPUT, in TB/s of 8 bytes
      per element;
  (3) torch-ROCm float32 on the same tensors, resident: torch.stft(center as the case says, pad_mode="reflect") -> re^2 + im^2 (torch's layout is bins before frames; the
      frames-major line adds .transpose(1, 2).contiguous()), and torch.fft.rfft on the framed signal is what it runs inside.
Each leg is a child process of this one, one at a time.
usage (GPU box): python tools/spectrum_time.py"""
import os
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.getcwd())

REPS, ROWS, L = 7, 4096, 16384
CASES = ((256, 64, False), (1024, 256, False), (400, 160, True), (512, 160, False))  # (n, hop, centred)


def median_ms(run):
    run()
    ts = sorted(run() / 3.0 for _ in range(REPS))
    return ts[REPS // 2], ts[0], ts[-1]


def infera_leg():
    from infera_amd import capi, onnx_writer as W

    dev = capi.device_ordinal(0)
    x = np.random.default_rng(1).standard_normal((ROWS, L)).astype(np.float32)
    d_in = capi.DeviceBuffer(dev, x.nbytes).upload(x)
    with tempfile.TemporaryDirectory() as td:
        for n, hop, centred in CASES:
            frames, bins = (L + (2 * (n // 2) if centred else 0) - n) // hop + 1, n // 2 + 1
            kw = dict(center=dict(pads=(n // 2, n // 2)), signal_rank=2) if centred else {}
            win = (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n) / n)).astype(np.float32)
            d_out = capi.DeviceBuffer(dev, 4 * ROWS * frames * bins)
            for layout in ("frames_major", "bins_major"):
                capi.load_model("spec", W.write(os.path.join(td, "spec.onnx"), W.stft_model(L=L, n=n, hop=hop, window=win, reader="pow",
                                                                                              transpose="after" if layout == "bins_major" else None, **kw)))
                s = capi.get_plan("spec")["plan"]["steps"]
                assert len(s) == 1 and s[0]["layout"] == layout, s
                t = median_ms(lambda: capi.time_predict_device("spec", d_in, ROWS, L, d_out, 3))
                tbs = 4.0 * ROWS * (L + frames * bins) / (t[0] * 1e-3) / 1e12
                print(f"infera   Spectrum n={n} hop={hop}{' centred' if centred else ''} {layout:<12} form {s[0]['form']:<8} {ROWS} x {L}: median {t[0]:7.3f} ms (min {t[1]:7.3f}, max {t[2]:7.3f}, n={REPS})  {tbs:5.2f} TB/s", flush=True)
                capi.unload_model("spec")
            cols = frames * bins
            nodes = [W.node("Relu", ["X"], ["out"], name="relu")]
            capi.load_model("elt", W.write(os.path.join(td, "elt.onnx"), W.model("elt", nodes, [], [W.value_info("X", ["N", cols])], [W.value_info("out", ["N", cols])])))
            e_in = capi.DeviceBuffer(dev, 4 * ROWS * cols)
            capi.synth_fill(e_in, 7, 0, ROWS, cols)
            t = median_ms(lambda: capi.time_predict_device("elt", e_in, ROWS, cols, d_out, 3))
            print(f"infera   elementwise pass (Relu) over {ROWS} x {cols}:                 median {t[0]:7.3f} ms (min {t[1]:7.3f}, max {t[2]:7.3f}, n={REPS})  {8.0 * ROWS * cols / (t[0] * 1e-3) / 1e12:5.2f} TB/s", flush=True)
            capi.unload_model("elt")
            e_in.free(), d_out.free()


def torch_leg():
    import torch

    if not torch.cuda.is_available():
        print(f"torch    NOT MEASURED: this torch build ({torch.__version__}) reports no usable GPU here", flush=True)
        return
    x = torch.from_numpy(np.random.default_rng(1).standard_normal((ROWS, L)).astype(np.float32)).cuda()
    for n, hop, centred in CASES:
        win = torch.hann_window(n, periodic=True, device="cuda")
        for layout in ("frames_major", "bins_major"):
            def f():
                s = torch.stft(x, n, hop, window=win, center=centred, pad_mode="reflect", return_complex=True)
                p = s.real ** 2 + s.imag ** 2
                return p.transpose(1, 2).contiguous() if layout == "frames_major" else p

            def run():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(3):
                    f()
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1)
            t = median_ms(run)
            print(f"torch    stft + power   n={n} hop={hop}{' centred' if centred else ''} {layout:<12}               {ROWS} x {L}: median {t[0]:7.3f} ms (min {t[1]:7.3f}, max {t[2]:7.3f}, n={REPS})", flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1:
        {"infera": infera_leg, "torch": torch_leg}[sys.argv[1]]()
    else:
        for leg in ("infera", "torch"):
            subprocess.run([sys.executable, os.path.abspath(__file__), leg], check=True, timeout=400)
