"""Mixed-radix frame lengths and centred frames of the Spectrum step without a GPU (INTEGRATION.md 2.6 "Spectral front ends"): the plan of the
torchaudio-shaped front end, the schedule, launch shape and index reciprocals of every served length, the new refusals, and the float32
evaluation of the centred log-mel model against a quarter of the project's bar."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from infera_amd import onnx_writer as W
from tests.test_spectrum import plan_of, signals, spectrogram_reference  # noqa: F401  (plan_of: the fixture)

SERVED = [2 * 2 ** a * 3 ** b * 5 ** c for a in range(11) for b in range(7) for c in range(5) if (b or c) and 4 <= 2 ** a * 3 ** b * 5 ** c <= 2048]
CENTRE = dict(pads=(200, 200), mode="reflect")


def centred_reference(w, x, dtype):
    """spectrogram_reference on the reflect-padded signal: what torch.stft(center=True, pad_mode="reflect") frames"""
    p = w["n"] // 2
    xp = np.pad(x, ((0, 0), (p, p)), mode="reflect")
    t = torch.tensor(x[:2], dtype=torch.float64)
    win = torch.tensor(w["window"], dtype=torch.float64)
    assert torch.equal(torch.stft(t, w["n"], w["hop"], window=win, center=True, pad_mode="reflect", return_complex=True),
                       torch.stft(torch.tensor(xp[:2], dtype=torch.float64), w["n"], w["hop"], window=win, center=False, return_complex=True))
    return spectrogram_reference(w, xp, dtype)


@pytest.mark.parametrize("spelling,rank,attr", [("NL", 2, False), ("NL", 3, False), ("N1L", 3, False), ("1NL", 2, False), ("NL", 2, True)])
def test_plan_of_the_centred_400_160_front_end(plan_of, spelling, rank, attr):
    plan = plan_of(W.stft_model(L=16000, n=400, hop=160, window=np.hanning(400), reader="pow", transpose="after",
                                center=dict(CENTRE, spelling=spelling, attr=attr), signal_rank=rank))
    assert [s["kind"] for s in plan["steps"]] == ["Spectrum"], plan["steps"]
    s = plan["steps"][0]
    assert (s["L"], s["frames"], s["bins"], s["pad_left"], s["pad_right"], s["pad_mode"], s["layout"]) == (16000, 101, 201, 200, 200, "reflect", "bins_major")
    radices, per_wave = s["form"].split("/")
    radices = [int(r) for r in radices.split(".")]
    assert set(radices) <= {2, 3, 4, 5, 8} and int(np.prod(radices)) == 200 and int(per_wave) == 3
    assert plan["output_shape"] == [-1, 201, 101]


def test_every_served_length_divides_exactly_and_fits(plan_of):
    """the (b * magic) >> 32 of every pass against b // d over every butterfly of a batch; the schedule; LDS within 160 KiB in both layouts"""
    assert len(SERVED) == 97 and {10, 400, 2916, 4050} <= set(SERVED)
    for n in SERVED:
        h, G = n // 2, -(-512 // (n // 2))
        for k, (hop, tr) in enumerate([(1, None), (n // 4, "after"), (n, None), (n + 3, "after")]):
            s = plan_of(W.stft_model(L=n + 30000 * hop, n=n, hop=hop, reader="pow", transpose=tr))["steps"][0]  # (frames beyond every run)
            assert s["lds_bytes"] <= 160 * 1024 and s["frames_per_group"] & (s["frames_per_group"] - 1) == 0, (n, hop, s)
            if k:
                continue
            assert s["form"] == ".".join(str(p["radix"]) for p in s["passes"]) + f"/{G}" and len(s["passes"]) <= 8
            ns = 1
            for p in s["passes"]:
                assert p["radix"] in (2, 3, 4, 5, 8) and p["ns"] == ns and p["hr"] * p["radix"] == h, (n, p)
                b = np.arange(G * p["hr"], dtype=np.uint64)
                assert p["hr"] == 1 or np.array_equal((b * np.uint64(p["magic_hr"])) >> np.uint64(32), b // np.uint64(p["hr"])), (n, p)
                j = np.arange(p["hr"], dtype=np.uint64)
                assert ns == 1 or np.array_equal((j * np.uint64(p["magic_ns"])) >> np.uint64(32), j // np.uint64(ns)), (n, p)
                ns *= p["radix"]
            assert ns == h


def test_power_of_two_plans_keep_their_form(plan_of):
    s = plan_of(W.stft_model(n=64, center=dict(pads=(32, 32)), signal_rank=2))["steps"][0]
    assert (s["form"], s["frames"], s["pad_left"], "passes" in s) == ("8.4/16", (256 + 64 - 64) // 16 + 1, 32, False)


REFUSALS = [
    (W.stft_model(L=2000, n=401), "stft", "STFT", "is odd"),
    (W.stft_model(L=2000, n=882), "stft", "STFT", "prime factor 7"),
    (W.stft_model(L=2000, n=44), "stft", "STFT", "prime factor 11"),
    (W.stft_model(center=dict(pads=(8, 8), mode="edge")), "pad", "Pad", 'mode = "edge"'),
    (W.stft_model(center=dict(pads=(8, 8), mode="wrap")), "pad", "Pad", 'mode = "wrap"'),
    (W.stft_model(center=dict(pads=(8, 8), mode="constant", value=1.0)), "pad", "Pad", "only zero padding"),
    (W.stft_model(center=dict(pads=(8, 8), rows=1)), "pad", "Pad", "only the time axis"),
    (W.stft_model(center=dict(pads=(-8, 8))), "pad", "Pad", "negative pads"),
    (W.stft_model(center=dict(pads=(256, 8))), "pad", "Pad", "at most L - 1"),
    (W.stft_model(center=dict(pads=(8, 8), nonconst=True)), "pad", "Pad", "pads is not a constant"),
    (W.stft_model(center=dict(pads=(8, 8), tap=True)), "pad", "Pad", "can only feed a Conv, or"),
    (W.stft_model(center=dict(pads=(8, 8)), elem=W.FLOAT16), "pad", "Pad", "float16"),
    (W.stft_model(center=dict(pads=(8, 8), quant=True)), "pad", "Pad", "quantised"),
]


@pytest.mark.parametrize("case", range(len(REFUSALS)))
def test_new_refusals_name_the_node(plan_of, case):
    blob, name, op, why = REFUSALS[case]
    with pytest.raises(Exception) as e:
        plan_of(blob)
    assert f"node '{name}' ({op}): unsupported operator form: " in str(e.value) and why in str(e.value), str(e.value)


def test_centred_log_mel_in_float32_stays_within_a_quarter_of_the_bar():
    _, w = W.spectrogram_model(L=1600, n=400, hop=160, mels=80, center=True)
    x = signals(5, 1600)
    ref, f32 = centred_reference(w, x, torch.float64), centred_reference(w, x, torch.float32)
    assert w["frames"] == 11 and np.all(np.abs(f32 - ref) <= 0.25 * (1e-4 * np.abs(ref) + 1e-6))
