"""Per-row sequence lengths (INTEGRATION.md section 2.6 "Padded windows") stated through the fixed-length definition of tests/recurrent_ref.py:
a row with length L gives what the same stack of layers gives when run on that row's first L steps alone.

recurrent_rows(spec, x, lens) runs recurrent_ref.recurrent on each row's prefix and assembles Y (zeros at t >= L), Y_h and Y_c.  Running the
whole STACK on the prefix is the same statement as running every layer with the lengths: layer 2 of a padded row reads layer 1's Y, which is
0 at t >= L, and does not read it there either.  The reverse direction of a prefix starts at step L - 1, which is the rule.  L = 0 is the
recurrence with no step: Y all zero, Y_h / Y_c the LAST layer's initial state (zero where the spec has none) -- ONNX Runtime accepts a length
of 0, torch's pack_padded_sequence refuses it; the kernel serves it.  numpy only: tests/test_recurrent_lens.py checks this module against
torch's pack_padded_sequence in float64 without a GPU, tests/test_recurrent_lens_gpu.py compares the kernel with it."""
from __future__ import annotations

import numpy as np

from tests import recurrent_ref as R


def recurrent_rows(spec, x, lens, dtype=np.float64):
    """x [N, T, F], lens [N] integers in 0 .. T -> (Y [N, T, D*H], Y_h [N, D*H], Y_c [N, D*H] or None) in `dtype`.  What lies at t >= lens[r]
    in x is never touched (it may be NaN)."""
    op, H, D = spec["op"], spec["H"], spec["D"]
    x = np.asarray(x)
    N, T, _ = x.shape
    lens = np.asarray(lens)
    assert lens.shape == (N,) and np.array_equal(lens, np.rint(lens)) and lens.min() >= 0 and lens.max() <= T, lens
    lens = lens.astype(np.int64)
    last = spec["layers"][-1]
    y = np.zeros((N, T, D * H), dtype)
    yh = np.zeros((N, D * H), dtype)
    yc = np.zeros((N, D * H), dtype) if op == "LSTM" else None
    if last.get("h0") is not None:
        yh[:] = np.asarray(last["h0"]).astype(dtype).reshape(1, D * H)
    if yc is not None and last.get("c0") is not None:
        yc[:] = np.asarray(last["c0"]).astype(dtype).reshape(1, D * H)
    for L in np.unique(lens):  # rows of one length run together: rows never mix, so this is each row alone
        if L == 0:
            continue
        at = np.nonzero(lens == L)[0]
        py, ph, pc = R.recurrent(spec, x[at, :L], dtype)
        y[at, :L], yh[at] = py, ph
        if yc is not None:
            yc[at] = pc
    return y, yh, yc


def with_lens(x, lens, dtype=np.float32):
    """the table of a call: [N, T*F + 1], the readings and the length column behind them"""
    x = np.asarray(x)
    return np.ascontiguousarray(np.concatenate([x.reshape(x.shape[0], -1), np.asarray(lens, dtype=np.float64).reshape(-1, 1)], axis=1).astype(dtype))


def fill_padding(x, lens, value):
    """a copy of x [N, T, F] with `value` at every t >= lens[r] of every row"""
    x = np.array(x, copy=True)
    for r, L in enumerate(np.asarray(lens).astype(np.int64)):
        x[r, L:] = value
    return x
