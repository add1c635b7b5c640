"""The float64 definition of the Spectrum step (INTEGRATION.md section 2.6 "Spectral front ends"): slice the frames, multiply the window,
numpy.fft in float64, then power / magnitude / layout."""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24


def hann(n):
    return (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n) / n)).astype(np.float32)


def stft(x, n, hop, window=None, onesided=True, mode="complex", bins_major=False):
    """x [..., L] -> [..., frames, bins (, 2)] (bins_major: [..., bins, frames (, 2)]) in float64."""
    x = np.asarray(x, np.float64)
    frames = (x.shape[-1] - n) // hop + 1
    idx = hop * np.arange(frames)[:, None] + np.arange(n)[None, :]
    fr = x[..., idx] * (np.ones(n) if window is None else np.asarray(window, np.float64))
    X = np.fft.rfft(fr, axis=-1) if onesided else np.fft.fft(fr, axis=-1)
    if mode == "complex":
        out = np.stack([X.real, X.imag], axis=-1)
        return np.swapaxes(out, -2, -3) if bins_major else out
    out = X.real ** 2 + X.imag ** 2
    if mode == "magnitude":
        out = np.sqrt(out)
    return np.swapaxes(out, -1, -2) if bins_major else out


def dft(x, n=None, onesided=True, mode="complex"):
    """x [..., L] zero-padded or truncated to n -> [..., bins (, 2)] in float64."""
    x = np.asarray(x, np.float64)
    n = x.shape[-1] if n is None else n
    x = x[..., :n] if x.shape[-1] >= n else np.concatenate([x, np.zeros(x.shape[:-1] + (n - x.shape[-1],))], axis=-1)
    return np.take(stft(x, n, n, None, onesided, mode), 0, axis=-3 if mode == "complex" else -2)


def frame_bound(ref_complex, n):
    """E per frame: 8 u log2(n) |ref|_2 over the frame's bins (ref_complex [..., bins, 2], frames-major)."""
    return 8.0 * U * np.log2(n) * np.sqrt((ref_complex ** 2).sum(axis=(-1, -2)))
