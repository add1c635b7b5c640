"""Spectral front ends without a GPU (INTEGRATION.md 2.6 "Spectral front ends"): the float64 reference against torch, the plan of every
served form, what is absorbed, every refusal, and the float32 evaluation of the two end-to-end models against a quarter of the project's bar."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from infera_amd import onnx_writer as W
from tests import spectrum_ref as R

HANN = np.hanning(65)[:64]


def signals(rows, L, seed=5):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((rows, L)) + 0.3 + np.cos(0.37 * np.arange(L))).astype(np.float32)


def spectrogram_reference(w, x, dtype):
    """torch evaluation of onnx_writer.spectrogram_model in `dtype`"""
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype)  # noqa: E731
    s = torch.stft(t(x), w["n"], w["hop"], window=t(w["window"]), center=False, return_complex=True)  # [N, bins, frames]
    pw = s.real ** 2 + s.imag ** 2
    if w["head"] == "cnn":
        img = torch.log(pw + t(w["eps"]))[:, None]
        c = torch.relu(torch.nn.functional.conv2d(img, t(w["conv_W"]), t(w["conv_b"]), padding=1))
        return (c.mean(dim=(2, 3)) @ t(w["head_W"]) + t(w["head_b"])).numpy()
    seq = torch.log(pw.transpose(1, 2) @ t(w["mel"]) + t(w["eps"]))
    H, Wi, Ri, B = w["hidden"], t(w["W"][0]), t(w["R"][0]), t(w["B"][0])
    h = c = torch.zeros(len(x), H, dtype=dtype)
    for k in range(seq.shape[1]):  # ONNX gate order i, o, f, c
        g = seq[:, k] @ Wi.T + h @ Ri.T + B[:4 * H] + B[4 * H:]
        i, o, f, cc = torch.sigmoid(g[:, :H]), torch.sigmoid(g[:, H:2 * H]), torch.sigmoid(g[:, 2 * H:3 * H]), torch.tanh(g[:, 3 * H:])
        c = f * c + i * cc
        h = o * torch.tanh(c)
    return (h @ t(w["head_W"]) + t(w["head_b"])).numpy()


def test_reference_agrees_with_torch():
    x = signals(3, 300).astype(np.float64)
    for onesided in (True, False):
        want = torch.view_as_real(torch.stft(torch.tensor(x), 64, 16, window=torch.tensor(HANN), center=False, onesided=onesided, return_complex=True)).numpy()
        got = R.stft(x, 64, 16, HANN, onesided, "complex", bins_major=True)
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    want = torch.view_as_real(torch.fft.rfft(torch.tensor(x), n=512)).numpy()
    assert np.abs(R.dft(x, 512) - want).max() <= 1e-12 * np.abs(want).max()


@pytest.fixture(scope="module")
def plan_of(built, tmp_path_factory):
    from infera_amd import capi

    def load(blob, name="spectrum_plan"):
        capi.load_model(name, W.write(str(tmp_path_factory.mktemp("spectrum") / f"{name}.onnx"), blob))
        try:
            return capi.get_plan(name)["plan"]
        finally:
            capi.unload_model(name)
    return load


PLANS = [
    (W.dft_model(L=64), "complex", "frames_major", [-1, 33, 2]),
    (W.dft_model(L=64, opset=20, axis=-2, onesided=0), "complex", "frames_major", [-1, 64, 2]),
    (W.dft_model(L=561, n=1024, reader="sumsq"), "power", "frames_major", [-1, 513]),
    (W.dft_model(L=64, C=3, axis=2, n=32, reader="l2", keepdims=1), "magnitude", "frames_major", [-1, 3, 17, 1]),
    (W.dft_model(L=64, reader="relu"), "complex", "frames_major", [-1, 33, 2]),
    (W.stft_model(), "complex", "frames_major", [-1, 13, 33, 2]),
    (W.stft_model(window=HANN, hop=70, onesided=0, reader="pow"), "power", "frames_major", [-1, 3, 64]),
    (W.stft_model(window=HANN, frame_length=True, reader="pow_sqrt", transpose="after"), "magnitude", "bins_major", [-1, 33, 13]),
    (W.stft_model(reader="sumsq", keepdims=1, transpose="after"), "power", "bins_major", [-1, 33, 13, 1]),
    (W.stft_model(transpose="before", reader="pow"), "power", "bins_major", [-1, 33, 13]),
    (W.stft_model(transpose="before"), "complex", "bins_major", [-1, 33, 13, 2]),
]


@pytest.mark.parametrize("case", range(len(PLANS)))
def test_plan_is_one_spectrum_step(plan_of, case):
    blob, mode, layout, shape = PLANS[case]
    plan = plan_of(blob)
    spec = [s for s in plan["steps"] if s["kind"] == "Spectrum"]
    assert len(spec) == 1 and (spec[0]["mode"], spec[0]["layout"]) == (mode, layout), plan["steps"]
    # the magnitude and transpose nodes emit nothing: only a reader that is neither (the Relu) adds a step
    assert len(plan["steps"]) == (2 if case == 4 else 1), plan["steps"]
    assert plan["output_shape"] == shape


REFUSALS = [
    (W.dft_model(inverse=1), "dft", "inverse = 1"),
    (W.dft_model(last=2), "dft", "complex input"),
    (W.dft_model(L=64, n=48), "dft", "not a power of two (not supported yet)"),
    (W.dft_model(L=64, n=4), "dft", "is below 8"),
    (W.dft_model(L=64, n=8192), "dft", "is above 4096"),
    (W.dft_model(L=64, C=3), "dft", "only the second to last axis"),
    (W.dft_model(nonconst="dft_length"), "dft", "dft_length is not a constant"),
    (W.stft_model(nonconst="frame_step"), "stft", "frame_step is not a constant"),
    (W.stft_model(nonconst="window"), "stft", "window is not a constant"),
    (W.stft_model(nonconst="frame_length"), "stft", "frame_length is not a constant"),
    (W.stft_model(window=HANN, frame_length=32), "stft", "the window has 64 values, frame_length is 32"),
    (W.stft_model(L=40, n=64), "stft", "no frame"),
    (W.stft_model(elem=W.FLOAT16), "stft", "float16"),
    (W.dft_model(time_major=True), "dft", "time-major"),
    (W.stft_model(L=1 << 22, n=4096, hop=1, onesided=0), "stft", "more than 2^31 elements per row"),
]


@pytest.mark.parametrize("case", range(len(REFUSALS)))
def test_refusals_name_the_node(plan_of, case):
    blob, name, why = REFUSALS[case]
    with pytest.raises(Exception) as e:
        plan_of(blob)
    op = "DFT" if name == "dft" else "STFT"
    assert f"node '{name}' ({op}): unsupported operator form: " in str(e.value) and why in str(e.value), str(e.value)


@pytest.mark.parametrize("head", ["lstm", "cnn"])
def test_float32_evaluation_stays_within_a_quarter_of_the_bar(head):
    _, w = W.spectrogram_model(head=head)
    x = signals(5, 400)
    ref, f32 = spectrogram_reference(w, x, torch.float64), spectrogram_reference(w, x, torch.float32)
    assert np.all(np.abs(f32 - ref) <= 0.25 * (1e-4 * np.abs(ref) + 1e-6))
