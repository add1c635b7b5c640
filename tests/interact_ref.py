"""float64 references and error bounds for the Interact step (INTEGRATION.md 2.6 "Feature interactions"), shared by the CPU and GPU tests.

T is a window [N, k, d]: k fields of d values per row.  u = 2^-24 is the unit roundoff of float32.

dot:  Z[n, i, j] = sum_c T[n, i, c] T[n, j, c].
    Bound (d + 2) u sum_c |a_c| |b_c|: the argument of dense_ref.py's docstring.  A sum of d products evaluated in float32 with every
    product and every partial sum rounded once (or products kept exact inside an fma) is off by at most gamma_d sum |a_c b_c| in ANY
    summation order, gamma_d = d u / (1 - d u); the two extra u cover the second-order terms for every d the step serves (d <= 256).

fm:   D[n, c] = (sum_f v_f)^2 - sum_f v_f^2 with v_f = T[n, f, c], then h * D, then optionally the sum over c.  Every partial sum and product
    is rounded once; write A = sum_f |v_f| and B = sum_f v_f^2.
      S  = fl(sum_f v_f), k - 1 additions in any order:        |S^ - S|   <= (k - 1) u A
      SS = fl(S^ * S^):  |S^2 - S^ 2| <= |S^ - S| (|S^| + |S|) <= 2 (k - 1) u A^2, and its own rounding adds u A^2:
                                                                |SS^ - S^2| <= (2 k - 1) u A^2
      Q  = fl(sum_f fl(v_f^2)), k products and k - 1 additions: |Q^ - Q|   <= k u B
      D  = fl(SS^ - Q^): the operands' errors plus u |SS^ - Q^| <= u (A^2 + B):
                                                                |D^ - D|   <= u (2 k A^2 + (k + 1) B)
      h D = fl(h * D^):  |h| times that plus u |h| |D^|:        |hD^ - hD| <= |h| u ((2 k + 1) A^2 + (k + 2) B)
    These are first-order counts; two more u on each term cover the second-order products ((k u)^2 terms with k <= 64):
                                                                E[n, c] = |h| u ((2 k + 3) A^2 + (k + 4) B)
    The sum over the d columns (d - 1 additions in any order) adds (d - 1) u sum_c |hD^_c| <= (d - 1) u |h| sum_c (A_c^2 + B_c) to
    sum_c E_c; two more u again: (d + 1).  Where the model multiplies by h AFTER that sum, the last multiply's own rounding moves behind the
    sum; it is bounded by the same u |h| sum_c (A_c^2 + B_c), which the (d + 1) already holds twice over, so one formula serves both.
    Results and partial results below the normal range (2^-126) are rounded to a multiple of 2^-149, an absolute error of at most 2^-150
    per operation that no relative bound covers: (3 k + d + 4) operations feed one output, each adding at most 2^-149 * max(1, |h|).
"""
import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -149
ROWS = (1, 63, 64, 65, 301, 2049)
KS = (2, 3, 15, 16, 17, 27, 32, 33, 64)   # the tile edges: 16 x 16 up to 16, 32 x 32 up to 32, four 32 x 32 tiles up to 64
DS = (1, 3, 4, 5, 16, 18, 130)            # the quad edges, one and several groups of columns


def dot_reference(T, sel=None):
    t = np.asarray(T, np.float64)
    z = np.einsum("nic,njc->nij", t, t)
    return z if sel is None else z.reshape(len(t), -1)[:, np.asarray(sel, np.int64)]


def dot_bound(T, sel=None):
    t = np.abs(np.asarray(T, np.float64))
    d = t.shape[2]
    with np.errstate(over="ignore", invalid="ignore"):
        b = (d + 2) * U * np.einsum("nic,njc->nij", t, t)
    return b if sel is None else b.reshape(len(t), -1)[:, np.asarray(sel, np.int64)]


def fm_reference(T, h=None, sum_last=False):
    t = np.asarray(T, np.float64)
    v = t.sum(axis=1) ** 2 - (t * t).sum(axis=1)
    if h is not None:
        v = v * float(h)
    return v.sum(axis=1, keepdims=True) if sum_last else v


def fm_bound(T, h=None, sum_last=False):
    t = np.asarray(T, np.float64)
    k, d = t.shape[1], t.shape[2]
    ah = 1.0 if h is None else abs(float(h))
    with np.errstate(over="ignore", invalid="ignore"):
        A2, B = np.abs(t).sum(axis=1) ** 2, (t * t).sum(axis=1)
        e = ah * U * ((2 * k + 3) * A2 + (k + 4) * B)
        floor = (3 * k + d + 4) * TINY * max(1.0, ah)
        if not sum_last:
            return e + floor
        return e.sum(axis=1, keepdims=True) + (d + 1) * U * ah * (A2 + B).sum(axis=1, keepdims=True) + floor


def exact_window(rows, k, d, seed=0):
    """integer values |v| <= 15: every product and partial sum is an integer far below 2^24 (dot: at most d * 225; fm: at most
    (15 k)^2 = 921,600 at k = 64), so float32 has one right answer in any evaluation order.  (The last-axis sum of fm multiplies that by d:
    exact_fm_ok says where it still is.)"""
    return np.random.default_rng(seed).integers(-15, 16, (rows, k, d)).astype(np.float32)


def exact_fm_ok(k, d, sum_last):
    """is every intermediate of the fm formula on exact_window an integer of at most 24 bits (then any evaluation order gives the same bits)?"""
    worst = (15 * k) ** 2
    return (worst * d if sum_last else worst) < 2 ** 24


def normal_window(rows, k, d, seed=0):
    """standard normal values; row 1 scaled by 1e18 and row 2 by 1e-18 (their products stay finite and, summed, normal)"""
    t = np.random.default_rng(seed).standard_normal((rows, k, d)).astype(np.float32)
    if rows > 2:
        t[1] *= np.float32(1e18)
        t[2] *= np.float32(1e-18)
    return t


def selections(k, seed=0):
    """the three index lists of the tests: DLRM's strict lower triangle, the triangle with the diagonal, and a shuffled list with duplicates
    and negative indices"""
    tri = np.asarray([i * k + j for i in range(k) for j in range(i)], np.int64)
    diag = np.asarray([i * k + j for i in range(k) for j in range(i + 1)], np.int64)
    rng = np.random.default_rng(seed + k)
    mixed = rng.integers(-k * k, k * k, min(k * k + 3, 97))
    mixed[0], mixed[-1] = -k * k, k * k - 1  # both ends of the range
    mixed[1] = mixed[2]                       # a duplicate for sure
    return {"triangle": tri, "diagonal": diag, "mixed": mixed.astype(np.int64)}


def within(got, ref, bound):
    """every element within its bound (a NaN / Inf reference wants the same class of value)"""
    got, ref, bound = (np.asarray(a, np.float64).reshape(-1) for a in (got, ref, bound))
    fin = np.isfinite(ref) & np.isfinite(bound)
    ok = np.abs(got[fin] - ref[fin]) <= bound[fin]
    return bool(np.all(ok)) and bool(np.all(~np.isfinite(got[~fin]) | ~np.isfinite(bound[~fin])))


def worst_over_bound(got, ref, bound):
    got, ref, bound = (np.asarray(a, np.float64).reshape(-1) for a in (got, ref, bound))
    fin = np.isfinite(ref) & np.isfinite(bound) & (bound > 0)
    return float(np.max(np.abs(got[fin] - ref[fin]) / bound[fin])) if fin.any() else 0.0
