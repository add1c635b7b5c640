"""The Spectrum step on the GPU (hip/spectrum.hip; INTEGRATION.md 2.6 "Spectral front ends") against tests/spectrum_ref.py.  Per frame of a
complex result: |got - ref|_2 <= E = 8 u log2(n) |ref|_2, u = 2^-24 (Higham's radix-2 bound, constant rounded up); power: |P - Pref| <=
E (2 sqrt(Pref) + E) + 4 u Pref; magnitude: |M - Mref| <= E + 2 u Mref.  The worst fraction per case is printed (SPECTRUM_RATIO; recorded
per n in profiles/spectrum_error_ratios.txt).  End to end: float64 torch at the project's bar 1e-4 |ref| + 1e-6."""
from __future__ import annotations

import numpy as np
import pytest

from infera_amd import onnx_writer as W
from tests import spectrum_ref as R
from tests.test_spectrum import signals, spectrogram_reference

pytestmark = pytest.mark.gpu

ROWS = 5
NS = [8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096]
MODES = {"complex": None, "power": "pow", "magnitude": "l2"}  # mode -> the reader the writer puts behind the transform
FORMS = dict(zip(NS, ["4/128", "8/64", "4.4/32", "8.4/16", "8.8/8", "8.4.4/4", "8.8.4/2", "8.8.8/1", "8.8.4.4/1", "8.8.8.4/1"]))


@pytest.fixture(scope="module")
def api(built):
    from infera_amd import capi

    assert capi.device_count() >= 1, capi.get_devices()
    return capi


def run(api, tmp_path, blob, x, name="spectrum", plan=None, resident=False):
    x = np.ascontiguousarray(x, np.float32)
    api.load_model(name, W.write(str(tmp_path / f"{name}.onnx"), blob))
    try:
        p = api.get_plan(name)["plan"]
        if plan is not None:
            plan.update(p)
        if not resident:
            return api.predict_from_blob(name, x.tobytes()).reshape(len(x), -1)  # (a rank-3 input: the blob entry)
        x = x.reshape(len(x), -1)
        per_row = int(np.prod(p["output_shape"][1:]))  # (one pass over the whole call)
        dev = api.device_ordinal(0)
        d_in, d_out = api.DeviceBuffer(dev, x.nbytes).upload(x), api.DeviceBuffer(dev, 4 * len(x) * per_row)
        api.predict_device(name, d_in, x.shape[0], x.shape[1], d_out)
        return d_out.download((len(x), per_row))
    finally:
        api.unload_model(name)


def check(got, x, n, hop, win, onesided, mode, bins_major):
    """the bound of the module docstring; returns the worst fraction of it"""
    ref = R.stft(x, n, hop, win, onesided, "complex")  # [rows, frames, bins, 2]
    E = R.frame_bound(ref, n)[..., None]
    want = R.stft(x, n, hop, win, onesided, mode)
    got = np.asarray(got, np.float64).reshape(R.stft(x, n, hop, win, onesided, mode, bins_major).shape)
    if bins_major:
        got = np.swapaxes(got, 1, 2)
    if mode == "complex":
        err, lim = np.sqrt(((got - want) ** 2).sum(axis=(-1, -2))), E[..., 0]
    elif mode == "power":
        err, lim = np.abs(got - want), E * (2 * np.sqrt(want) + E) + 4 * R.U * want
    else:
        err, lim = np.abs(got - want), E + 2 * R.U * want
    ratio = float((err / lim).max())
    print(f"SPECTRUM_RATIO n={n} hop={hop} mode={mode} {ratio:.4f}")
    assert ratio <= 1.0, ratio
    return ratio


@pytest.mark.parametrize("n,j", [(n, j) for n in NS for j in range(4)])
def test_stft_within_the_bound(api, tmp_path, n, j):
    i = NS.index(n)
    hop = [1, n // 4, n, n + 3][j]
    onesided, mode, bins_major = (i + j) % 2, list(MODES)[(i + j) % 3], bool(((i + j) // 2) % 2)
    frames = 256 * max(1, 512 // (n // 2)) + 3  # odd and beyond the largest run: neither 1 nor a multiple of Fw
    L = n + (frames - 1) * hop + (hop - 1) // 2
    x = signals(ROWS, L, seed=n + j)
    plan = {}
    tr = None if not bins_major else "after" if mode != "complex" else "before"
    blob = W.stft_model(L=L, n=n, hop=hop, window=R.hann(n), onesided=onesided, reader=MODES[mode], transpose=tr)
    got = run(api, tmp_path, blob, x, plan=plan)
    s = plan["steps"][0]
    assert (s["frames"], s["form"], s["layout"]) == (frames, FORMS[n], "bins_major" if bins_major else "frames_major")
    assert frames > s["frames_per_group"] and frames % s["frames_per_group"] != 0
    check(got, x, n, hop, R.hann(n), bool(onesided), mode, bins_major)


def test_forms_are_all_the_host_selects(api, tmp_path):
    seen = set()
    for n in NS:
        plan = {}
        run(api, tmp_path, W.stft_model(L=2 * n, n=n, hop=n), signals(1, 2 * n), plan=plan)
        seen.add(plan["steps"][0]["form"])
    assert seen == set(FORMS.values())


@pytest.mark.parametrize("L,n,C", [(561, 1024, None), (700, 256, None), (64, 64, 3), (100, 128, 3)])
def test_dft_padded_truncated_and_channels(api, tmp_path, L, n, C):
    x = signals(ROWS * (C or 1), L).reshape((ROWS, C, L) if C else (ROWS, L))
    for mode in MODES:
        got = run(api, tmp_path, W.dft_model(L=L, n=n, C=C, axis=2 if C else None, reader=MODES[mode]), x)
        xp = np.pad(x[..., :n], [(0, 0)] * (x.ndim - 1) + [(0, max(0, n - L))])
        check(got, xp.reshape(-1, n), n, n, None, True, mode, False)


def test_exact_values(api, tmp_path):
    n = 64
    rng = np.random.default_rng(3)
    x = np.stack([np.ones(n), np.zeros(n), rng.integers(-8, 9, n), rng.integers(-8, 9, n)]).astype(np.float32)
    got = run(api, tmp_path, W.dft_model(L=n, onesided=0), x).reshape(4, n, 2)
    assert got[0, 0, 0] == n and np.count_nonzero(got[0]) == 1 and not got[1].view(np.uint32).any()  # (row 1: +0 everywhere)
    for r in (2, 3):
        assert got[r, 0, 0] == x[r].sum() and got[r, n // 2, 0] == (x[r][0::2] - x[r][1::2]).sum() and got[r, 0, 1] == 0 and got[r, n // 2, 1] == 0


def test_same_bits_across_rows_positions_and_layouts(api, tmp_path):
    n, hop, f = 256, 64, 21
    L = n + 40 * hop
    x = signals(257, L)
    win = R.hann(n)
    blob = W.stft_model(L=L, n=n, hop=hop, window=win, reader="pow")
    many = run(api, tmp_path, blob, x, resident=True)
    alone = run(api, tmp_path, blob, x[100:101])
    assert many[100].tobytes() == alone[0].tobytes()
    shifted = np.zeros_like(x[:1])
    shifted[0, :L - f * hop] = x[100, f * hop:]
    moved = run(api, tmp_path, blob, shifted).reshape(41, -1)
    assert moved[0].tobytes() == alone.reshape(41, -1)[f].tobytes()
    major = run(api, tmp_path, W.stft_model(L=L, n=n, hop=hop, window=win, reader="pow", transpose="after"), x[100:101])
    assert major.reshape(-1, 41).T.tobytes() == alone.tobytes()


def test_nan_stays_in_its_frames_and_row(api, tmp_path):
    n, hop, at = 64, 16, 200
    L = n + 30 * hop
    x = signals(ROWS, L)
    x[2, at] = np.nan
    got = run(api, tmp_path, W.stft_model(L=L, n=n, hop=hop, window=R.hann(n) + 0.1, reader="pow"), x).reshape(ROWS, 31, -1)
    hit = np.array([f * hop <= at < f * hop + n for f in range(31)])
    assert np.isnan(got[2, hit]).all() and not np.isnan(got[2, ~hit]).any() and not np.isnan(np.delete(got, 2, axis=0)).any()


def test_long_call_beyond_two_grid_strides(api, tmp_path):
    n, L, rows = 8, 40, 2 * 2048 + 37  # one (signal, run) unit per row; the grid is capped at 2048 work groups
    x = signals(rows, L)
    got = run(api, tmp_path, W.stft_model(L=L, n=n, hop=8), x, resident=True)
    check(got[-50:], x[-50:], n, 8, None, True, "complex", False)


@pytest.mark.parametrize("head", ["lstm", "cnn"])
def test_spectrogram_models_against_float64(api, tmp_path, head):
    import torch

    blob, w = W.spectrogram_model(head=head)
    x = signals(ROWS, 400)
    got, ref = run(api, tmp_path, blob, x), spectrogram_reference(w, x, torch.float64)
    assert np.all(np.abs(got - ref) <= 1e-4 * np.abs(ref) + 1e-6), np.abs(got - ref).max()
