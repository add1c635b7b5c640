"""The references and bounds of tests/interact_ref.py, checked before any kernel meets them: the float64 references agree with a plain
np.einsum restatement, and a float32 numpy evaluation stays inside the bound in three different summation orders on the inputs the GPU
test uses (tests/test_interact_gpu.py)."""
import numpy as np
import pytest

import interact_ref as R

BOUNDED = [(3, 4), (16, 5), (17, 16), (27, 16), (33, 18)]  # (k, d) of the bounded GPU cases


def test_references_agree_with_einsum():
    t = R.normal_window(7, 5, 6, seed=1).astype(np.float64)
    z = np.einsum("nkd,njd->nkj", t, t)
    assert np.allclose(R.dot_reference(t), z, rtol=1e-13, atol=0)
    sel = R.selections(5)["mixed"]
    assert np.allclose(R.dot_reference(t, sel), z.reshape(7, 25)[:, sel], rtol=1e-13, atol=0)
    # the written formula equals twice the sum over the pairs i < j
    pairs = 2 * sum(t[:, i] * t[:, j] for i in range(5) for j in range(i))
    scale = np.einsum("nkd->nd", np.abs(t)) ** 2
    assert np.all(np.abs(R.fm_reference(t) - pairs) <= 1e-13 * scale)
    assert np.all(np.abs(R.fm_reference(t, 0.5, True) - 0.5 * pairs.sum(axis=1, keepdims=True)) <= 1e-13 * scale.sum(axis=1, keepdims=True))


def test_exact_windows_have_one_answer():
    t = R.exact_window(9, 64, 130, seed=2)
    z = R.dot_reference(t)
    assert np.array_equal(z.astype(np.float32).astype(np.float64), z) and np.abs(z).max() < 2 ** 24
    assert R.exact_fm_ok(64, 130, False) and not R.exact_fm_ok(64, 130, True) and R.exact_fm_ok(64, 16, True)


def _sum32(x, axis, order):
    """float32 sum along `axis`, every partial sum rounded: ascending, descending, or pairwise"""
    x = np.moveaxis(np.asarray(x, np.float32), axis, 0)
    if order == "pairwise":
        while len(x) > 1:
            if len(x) % 2:
                x = np.concatenate([x, np.zeros_like(x[:1])])
            x = x[0::2] + x[1::2]
        return x[0]
    acc = np.zeros_like(x[0])
    for v in (x if order == "up" else x[::-1]):
        acc = acc + v
    return acc


@pytest.mark.parametrize("order", ["up", "down", "pairwise"])
@pytest.mark.parametrize("k,d", BOUNDED)
def test_float32_stays_inside_the_bounds(k, d, order):
    t = R.normal_window(65, k, d, seed=k + d)
    with np.errstate(over="ignore", invalid="ignore"):
        z = _sum32(t[:, :, None, :] * t[:, None, :, :], 3, order)
        assert R.within(z, R.dot_reference(t), R.dot_bound(t)), R.worst_over_bound(z, R.dot_reference(t), R.dot_bound(t))
        s = _sum32(t, 1, order)
        dd = s * s - _sum32(t * t, 1, order)
        for h in (None, 0.5):
            v = dd if h is None else dd * np.float32(h)
            assert R.within(v, R.fm_reference(t, h), R.fm_bound(t, h)), R.worst_over_bound(v, R.fm_reference(t, h), R.fm_bound(t, h))
            tot = _sum32(v, 1, order)[:, None]
            assert R.within(tot, R.fm_reference(t, h, True), R.fm_bound(t, h, True))
            if h is not None:  # the multiply behind the sum
                tot = (_sum32(dd, 1, order) * np.float32(h))[:, None]
                assert R.within(tot, R.fm_reference(t, h, True), R.fm_bound(t, h, True))


def test_bounds_are_not_loose_by_orders_of_magnitude():
    """a bound nobody can miss checks nothing: float32 uses a visible share of each (more than 1/200 on these sizes)"""
    t = R.normal_window(301, 27, 16, seed=5)
    z = _sum32(t[:, :, None, :] * t[:, None, :, :], 3, "up")
    assert R.worst_over_bound(z, R.dot_reference(t), R.dot_bound(t)) > 0.005
    s = _sum32(t, 1, "up")
    assert R.worst_over_bound(s * s - _sum32(t * t, 1, "up"), R.fm_reference(t), R.fm_bound(t)) > 0.005
