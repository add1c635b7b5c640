"""Mixed-radix frame lengths and centred frames of the Spectrum step on the GPU (hip/spectrum.hip; INTEGRATION.md 2.6 "Spectral front ends"),
against tests/spectrum_ref.py with the bound of tests/test_spectrum_gpu.py, unchanged: per frame |got - ref|_2 <= 8 u log2(n) |ref|_2 (log2 n
no longer an integer).  The worst fraction per case is printed (SPECTRUM_RATIO; recorded per n in profiles/spectrum_mixed_error_ratios.txt)."""
from __future__ import annotations

import numpy as np
import pytest

from infera_amd import onnx_writer as W
from tests import spectrum_ref as R
from tests.test_spectrum import signals
from tests.test_spectrum_gpu import MODES, ROWS, api, check, run  # noqa: F401  (api: the fixture)
from tests.test_spectrum_mixed import centred_reference

pytestmark = pytest.mark.gpu

NS = [10, 12, 20, 24, 30, 36, 50, 60, 96, 100, 150, 200, 360, 400, 480, 750, 1000, 1536, 2250, 2916, 3000, 3840, 4050]
SPELLINGS = [("NL", 2), ("N1L", 3), ("1NL", 2), ("NL", 3)]


@pytest.mark.parametrize("n,j", [(n, j) for n in NS for j in range(4)])
def test_stft_within_the_bound(api, tmp_path, n, j):
    i = NS.index(n)
    hop = [1, n // 4, n, n + 3][j]
    onesided, mode, bins_major = (i + j) % 2, list(MODES)[(i + j) % 3], bool(((i + j) // 2) % 2)
    frames = 256 * -(-512 // (n // 2)) + 3  # odd and beyond the largest run: neither 1 nor a multiple of Fw
    L = n + (frames - 1) * hop + (hop - 1) // 2
    x = signals(ROWS, L, seed=n + j)
    plan = {}
    tr = None if not bins_major else "after" if mode != "complex" else "before"
    got = run(api, tmp_path, W.stft_model(L=L, n=n, hop=hop, window=R.hann(n), onesided=onesided, reader=MODES[mode], transpose=tr), x, plan=plan)
    s = plan["steps"][0]
    assert (s["frames"], s["layout"], len(s["passes"]) > 0) == (frames, "bins_major" if bins_major else "frames_major", True)
    assert frames > s["frames_per_group"] and frames % s["frames_per_group"] != 0
    check(got, x, n, hop, R.hann(n), bool(onesided), mode, bins_major)


@pytest.mark.parametrize("n", [60, 100])
def test_exact_values(api, tmp_path, n):
    rng = np.random.default_rng(3)
    x = np.stack([np.ones(n), np.zeros(n), rng.integers(-8, 9, n), rng.integers(-8, 9, n)]).astype(np.float32)
    got = run(api, tmp_path, W.stft_model(L=n, n=n, hop=n, onesided=0), x).reshape(4, n, 2)
    bits = got[:2].reshape(2, -1).view(np.uint32)
    assert got[0, 0, 0] == n and not bits[0, 1:].any() and not bits[1].any()  # (+0 everywhere else, and in the zero row)
    for r in (2, 3):
        assert got[r, 0, 0] == x[r].sum() and got[r, n // 2, 0] == (x[r][0::2] - x[r][1::2]).sum() and got[r, 0, 1] == 0 and got[r, n // 2, 1] == 0


@pytest.mark.parametrize("n", [64, 400])
@pytest.mark.parametrize("case", range(9))
def test_centred_is_the_explicitly_padded_signal(api, tmp_path, n, case):
    pl, pr, mode = [(n // 2, n // 2, "reflect"), (3, 0, "reflect"), (n // 2, n // 2, "constant")][case % 3]
    # 16-byte loads in interior runs (where the left pad allows it); word loads; frames staged one by one (hop = n), 16-byte loads again
    L, hop = [(16000, n // 4), (16001, n // 4 + 1), (32000, n)][case // 3]
    x = signals(3, L, seed=case)
    spelling, rank = SPELLINGS[case % 4]
    plan = {}
    got = run(api, tmp_path, W.stft_model(L=L, n=n, hop=hop, window=R.hann(n), center=dict(pads=(pl, pr), mode=mode, spelling=spelling), signal_rank=rank), x, plan=plan)
    s = plan["steps"][0]
    assert s["frames"] > 2 * s["frames_per_group"] and (s["pad_left"], s["pad_right"], s["pad_mode"]) == (pl, pr, mode)  # (edge runs and interior runs)
    xp = np.pad(x, ((0, 0), (pl, pr)), mode=mode)
    want = run(api, tmp_path, W.stft_model(L=L + pl + pr, n=n, hop=hop, window=R.hann(n)), xp)
    assert got.tobytes() == want.tobytes()


def test_same_bits_across_rows_positions_and_layouts(api, tmp_path):
    n, hop, f, L = 400, 160, 7, 6400
    x = signals(257, L)
    kw = dict(L=L, n=n, hop=hop, window=R.hann(n), reader="pow", center=dict(pads=(200, 200)), signal_rank=2)
    many = run(api, tmp_path, W.stft_model(**kw), x, resident=True)
    alone = run(api, tmp_path, W.stft_model(**kw), x[100:101])
    assert many[100].tobytes() == alone[0].tobytes()
    major = run(api, tmp_path, W.stft_model(transpose="after", **kw), x[100:101])
    assert major.reshape(201, -1).T.tobytes() == alone.tobytes()
    plain = dict(kw, center=None, signal_rank=3)
    shifted = np.zeros_like(x[:1])
    shifted[0, :L - f * hop] = x[100, f * hop:]
    here, moved = run(api, tmp_path, W.stft_model(**plain), x[100:101]).reshape(-1, 201), run(api, tmp_path, W.stft_model(**plain), shifted).reshape(-1, 201)
    assert moved[0].tobytes() == here[f].tobytes()


def test_nan_stays_in_its_frames_and_row(api, tmp_path):
    n, hop, L, pl = 400, 160, 6400, 200
    x = signals(ROWS, L)
    x[2, 1] = np.nan
    got = run(api, tmp_path, W.stft_model(L=L, n=n, hop=hop, window=R.hann(n) + 0.1, reader="pow", center=dict(pads=(pl, pl)), signal_rank=2), x).reshape(ROWS, 41, -1)
    hit = np.array([any(f * hop <= p < f * hop + n for p in (pl - 1, pl + 1)) for f in range(41)])
    assert hit.any() and np.isnan(got[2, hit]).all() and not np.isnan(got[2, ~hit]).any() and not np.isnan(np.delete(got, 2, axis=0)).any()


def test_centred_log_mel_model_against_float64(api, tmp_path):
    import torch

    blob, w = W.spectrogram_model(L=1600, n=400, hop=160, mels=80, center=True)
    x = signals(ROWS, 1600)
    got, ref = run(api, tmp_path, blob, x), centred_reference(w, x, torch.float64)
    assert np.all(np.abs(got - ref) <= 1e-4 * np.abs(ref) + 1e-6), np.abs(got - ref).max()
