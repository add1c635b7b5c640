"""Padded token sequences on the GPU (hip/attention.hip attention_kernel<DT, true>, hip/layernorm.hip mean_time_masked_kernel; INTEGRATION.md
section 2.6 "Padded sequences"): attention under a row's own key mask and the masked mean over time against tests/padded_ref.py at the
project's bar 1e-4 |ref| + 1e-6 per element (attention_ref.verdict), the exact statements of the rule as bit comparisons, a whole text
encoder against its float64 restatement, and bit-identity between the call paths.

Which rows are fair cases (tests/test_padded.py::test_float32_is_a_fair_case_where_a_key_is_kept; attention_ref.attention32 on the CPU):
with a kept key in every row float32 itself sits at 0.04 of the bar under every fill.  A row WITHOUT a kept key sits at 0.007 under
finfo.min and -1e9 (the fill absorbs the score: equal rounded scores), but at 5.7 / 19 under -10000 / -65504, where the rounded score keeps
one ulp of the product's rounding: so such rows appear only under finfo.min and -1e9 (expected: the mean of V) and under -inf (expected:
NaN), and under the bias fill -10000 every row keeps a key."""
from __future__ import annotations

import threading

import numpy as np
import pytest

from infera_amd import onnx_writer as W
from tests import attention_ref as A
from tests import padded_ref as P

pytestmark = pytest.mark.gpu

FMIN = P.FMIN
NEG_INF = float("-inf")
PAD = 3


@pytest.fixture(scope="module")
def api(built):
    from infera_amd import capi

    assert capi.device_count() >= 1, capi.get_devices()
    return capi


class Loaded:
    def __init__(self, api, tmp_path, blob, name, select=""):
        self.api, self.name = api, name
        api.load_model(name, W.write(str(tmp_path / f"{name}.onnx"), blob) + select)

    def __enter__(self):
        return lambda x: self.api.predict(self.name, np.ascontiguousarray(x, np.float32))

    def __exit__(self, *exc):
        self.api.unload_model(self.name)


def run(api, tmp_path, blob, x, name="padded", select=""):
    with Loaded(api, tmp_path, blob, name, select) as f:
        return f(x)


def table(q, k, v, cols):
    """the call's table: the packed window [rows, T 3E] and the mask's columns behind it"""
    return np.ascontiguousarray(np.concatenate([A.pack(q, k, v), cols], axis=1), np.float32)


# ---- attention alone -------------------------------------------------------------------------------------------------------------------

SHAPES = [(1, 4, 1), (7, 5, 5), (16, 16, 2), (17, 16, 2), (33, 16, 2), (48, 4, 3), (65, 64, 2), (128, 16, 8), (128, 128, 1), (1024, 4, 5)]
# (form, fill, source, a row without a kept key)
VARIANTS = [("add", FMIN, "mask", True), ("add", -10000.0, "mask", False), ("add", -1e9, "mask", True), ("replace", FMIN, "mask", True),
            ("replace", NEG_INF, "mask", True), ("add", FMIN, "ids", True), ("replace", NEG_INF, "ids", True), ("add", -10000.0, "ids", False)]
_cases = {}


def attention_case(shape, none_kept):
    """(q, k, v, keep) of a shape, drawn once: 37 rows (3 at T = 1024, the 32-word bitmap) through the patterns; none_kept: the last row
    keeps no key"""
    key = (shape, none_kept)
    if key not in _cases:
        T, dh, h = shape
        rows = 3 if T >= 512 else 37
        q, k, v = A.unit_case(T, dh * h, rows, seed=11)
        keep = P.keep_rows(T, rows) if T < 512 else np.stack([P.pattern(n, T, np.random.default_rng(T)) for n in ("left33", "holes", "tile")])
        if none_kept:
            keep = keep.copy()
            keep[-1] = False
        _cases[key] = (q, k, v, keep)
    return _cases[key]


_refs = {}


def attention_ref_of(shape, none_kept, form, fill):
    key = (shape, none_kept, form, fill)
    if key not in _refs:
        q, k, v, keep = attention_case(shape, none_kept)
        _refs[key] = P.attention_rows(q, k, v, shape[2], 1.0 / np.sqrt(shape[1]), keep, fill, form)
    return _refs[key]


@pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: "%s_%s_%s" % (v[0], {FMIN: "fmin", NEG_INF: "-inf"}.get(v[1], v[1]), v[2]))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda c: "T%d_dh%d_h%d" % c)
def test_attention_under_row_masks(api, tmp_path, shape, variant):
    T, dh, h = shape
    form, fill, source, none_kept = variant
    q, k, v, keep = attention_case(shape, none_kept)
    ref = attention_ref_of(shape, none_kept, form, fill)
    cols = P.mask_columns(keep, source, PAD, np.random.default_rng(T))
    blob = W.attention_only(T, dh * h, h, row_mask=dict(form=form, fill=fill, from_ids=PAD if source == "ids" else None))
    got = run(api, tmp_path, blob, table(q, k, v, cols))
    r = P.verdict(got, ref)
    print(f"\nrow-masked attention T={T} dh={dh} h={h} {form} fill={fill} {source}: {r:.4f} of the bar")
    assert r <= 1.0, r
    if none_kept:
        if fill == NEG_INF:
            assert np.isnan(got[-1]).all() and not np.isnan(got[:-1]).any()
        else:  # the mean of V over all T keys
            assert P.verdict(got[-1], np.broadcast_to(v[-1].astype(np.float64).mean(axis=0), (T, dh * h))) <= 1.0


def test_row_without_a_kept_key_changes_no_other_row(api, tmp_path):
    """-inf: every query of that row is NaN; every other row has the bits of the run in which that row keeps all its keys"""
    shape = (48, 4, 3)
    T, dh, h = shape
    q, k, v, keep = attention_case(shape, True)
    with Loaded(api, tmp_path, W.attention_only(T, dh * h, h, row_mask=dict(form="replace", fill=NEG_INF)), "nokey") as f:
        got = f(table(q, k, v, keep.astype(np.float32)))
        full = keep.copy()
        full[-1] = True
        other = f(table(q, k, v, full.astype(np.float32)))
    assert np.isnan(got[-1]).all() and np.array_equal(got[:-1], other[:-1]) and not np.isnan(other).any()


@pytest.mark.parametrize("fill", [FMIN, -10000.0, -1e9], ids=["fmin", "-1e4", "-1e9"])
@pytest.mark.parametrize("shape", [(33, 16, 2), (128, 16, 8)], ids=lambda c: "T%d_dh%d_h%d" % c)
def test_all_keys_kept_is_the_unmasked_model(api, tmp_path, shape, fill):
    T, dh, h = shape
    q, k, v = A.unit_case(T, dh * h, 37, seed=13)
    plain = run(api, tmp_path, W.attention_only(T, dh * h, h), A.pack(q, k, v), name="plain")
    masked = run(api, tmp_path, W.attention_only(T, dh * h, h, row_mask=dict(form="add", fill=fill)), table(q, k, v, np.ones((37, T), np.float32)), name="kept")
    assert np.array_equal(masked, plain)


@pytest.mark.parametrize("form,fill", [("add", FMIN), ("replace", FMIN), ("replace", NEG_INF)], ids=["add_fmin", "replace_fmin", "replace_-inf"])
def test_right_padded_row_is_the_shorter_model(api, tmp_path, form, fill):
    """an excluded key is a key beyond T: steps [:L] of a row right-padded to L have the bits of the T = L unmasked model on its first L steps"""
    T, dh, h, rows = 48, 16, 2, 5
    q, k, v = A.unit_case(T, dh * h, rows, seed=17)
    with Loaded(api, tmp_path, W.attention_only(T, dh * h, h, row_mask=dict(form=form, fill=fill)), "long") as f:
        for L in (1, 16, 17, 33):
            keep = np.zeros((rows, T), np.float32)
            keep[:, :L] = 1
            got = f(table(q, k, v, keep)).reshape(rows, T, dh * h)
            short = run(api, tmp_path, W.attention_only(L, dh * h, h), A.pack(q[:, :L], k[:, :L], v[:, :L]), name=f"short{L}").reshape(rows, L, dh * h)
            assert np.array_equal(got[:, :L], short), L


def test_nan_at_a_masked_step(api, tmp_path):
    """excluding fill: a masked key is never read, so a NaN in K and V there does not reach the row, in a tile it shares with kept keys
    or not; under the bias fill -10000 every key is read and every product formed: the NaN of K makes its head NaN in that row, the NaN
    of V its column of its head, and nothing else changes (attention_ref.NONFINITE)"""
    T, dh, h, rows = 65, 16, 2, 7
    E = dh * h
    q, k, v = A.unit_case(T, E, rows, seed=19)
    keep = np.ones((rows, T), np.float32)
    keep[:, 20] = 0   # shares its tile with kept keys
    keep[:, 32:64] = 0  # a wholly masked tile
    kb, vb = k.copy(), v.copy()
    for step in (20, 40):
        kb[3, step, 5] = np.nan       # head 0
        vb[3, step, dh + 2] = np.nan  # head 1, column 2
    for form, fill in (("add", FMIN), ("replace", NEG_INF)):
        with Loaded(api, tmp_path, W.attention_only(T, E, h, row_mask=dict(form=form, fill=fill)), "excl") as f:
            assert np.array_equal(f(table(q, kb, vb, keep)), f(table(q, k, v, keep))), form
    with Loaded(api, tmp_path, W.attention_only(T, E, h, row_mask=dict(form="add", fill=-10000.0)), "bias") as f:
        clean, got = f(table(q, k, v, keep)).reshape(rows, T, E), f(table(q, kb, vb, keep)).reshape(rows, T, E)
    want_nan = np.zeros((rows, T, E), bool)
    want_nan[3, :, :dh] = True
    want_nan[3, :, dh + 2] = True
    assert np.array_equal(np.isnan(got), want_nan) and np.array_equal(got[~want_nan], clean[~want_nan]) and not np.isnan(clean).any()


# ---- masked mean -----------------------------------------------------------------------------------------------------------------------

def mean_graph(T, E, **kw):
    nodes, inits = [W.node("Reshape", ["X", "s"], ["x3"])], [W.tensor("s", np.asarray([-1, T, E], np.int64))]
    out = W.masked_mean_nodes(nodes, inits, "mm_", "x3", "M", T, E, **kw)
    return W.model("mm", nodes, inits, [W.value_info("X", ["N", T * E]), W.value_info("M", ["N", T], W.INT64)], [W.value_info(out, ["N", E])], opset=20)


@pytest.mark.parametrize("T,E", [(7, 3), (24, 64), (128, 128)])
@pytest.mark.parametrize("source", ["mask", "ids"])
def test_masked_mean(api, tmp_path, T, E, source):
    rows = len(P.PATTERNS) + 1
    x = np.random.default_rng(T).uniform(-1, 1, (rows, T, E)).astype(np.float32)
    keep = P.keep_rows(T, rows)
    keep[-1] = False  # no kept step: 0 / clip = 0
    cols = P.mask_columns(keep, source, PAD, np.random.default_rng(E))
    kw = dict(from_ids=PAD, expand="shape") if source == "ids" else dict(count="mask")
    with Loaded(api, tmp_path, mean_graph(T, E, **kw), "mm") as f:
        got = f(np.concatenate([x.reshape(rows, -1), cols], axis=1))
        r = P.verdict(got, P.masked_mean(x, keep, 1e-9))
        print(f"\nmasked mean T={T} E={E} {source}: {r:.4f} of the bar")
        assert r <= 1.0 and np.array_equal(got[-1], np.zeros(E, np.float32))
        # a masked step is not read
        xb = x.copy()
        xb[~keep] = np.nan
        assert np.array_equal(f(np.concatenate([xb.reshape(rows, -1), cols], axis=1)), got)
        # a row right-padded to L is MeanTime of the T = L model, bit for bit
        for L in sorted({1, min(T, 5), min(T, 17), T}):
            kl = np.zeros((rows, T), bool)
            kl[:, :L] = True
            padded = f(np.concatenate([x.reshape(rows, -1), P.mask_columns(kl, source, PAD, np.random.default_rng(L))], axis=1))
            short = run(api, tmp_path, A.mean_time_graph(L, E, 0), x[:, :L].reshape(rows, -1), name=f"mt{L}")
            assert np.array_equal(padded, short), L


# ---- the whole text encoder ------------------------------------------------------------------------------------------------------------

# (spec, weight scale of every Linear).  The reference evaluated in float32 numpy against float64 (CPU; worst of both heads over the 256
# rows below), the fair-case rule of tests/test_transformer_gpu.py (a quarter of the bar):
#   T = 16, V = 50, E = 32, h = 4, ff = 64, L = 2     weights x 1: first 0.096, sentence 0.040 (the same under every fill)
#   T = 128, V = 50, E = 64, h = 4, ff = 128, L = 1   weights x 1: first 0.104, sentence 0.014
# Both are inside the quarter at default weights, so no Linear is scaled down.
ENCODERS = [(dict(T=16, V=50, E=32, h=4, ff=64, layers=2), 1.0), (dict(T=128, V=50, E=64, h=4, ff=128, layers=1), 1.0)]


def encoder_lengths(T, rows, seed=0):
    rng = np.random.default_rng([seed, T])
    fixed = [T, 1, 2, 15, 16, 17, 31, 32, 33]
    return np.asarray([min(T, fixed[r]) if r < len(fixed) else int(rng.integers(1, T + 1)) for r in range(rows)])


@pytest.mark.parametrize("kw", [dict(form="add", fill=FMIN), dict(form="replace", fill=NEG_INF, from_ids=True, expand="shape"), dict(form="add", fill=-10000.0)],
                         ids=["bert", "distilbert-ids", "bias-1e4"])
@pytest.mark.parametrize("cfg,scale", ENCODERS, ids=["T16_L2", "T128_L1"])
def test_text_encoder_against_float64(api, tmp_path, cfg, scale, kw):
    spec = W.text_encoder_spec(weight_scale=scale, **cfg)
    rows = 256
    ids, keep, both, only_ids = W.text_encoder_inputs(spec, encoder_lengths(cfg["T"], rows), seed=1)
    ref = W.text_encoder_reference(spec, ids, keep, kw["form"], kw["fill"])
    ref32 = W.text_encoder_reference(spec, ids, keep, kw["form"], kw["fill"], dtype=np.float32)
    blob = W.text_encoder_from_spec(spec, **kw)
    x = only_ids if kw.get("from_ids") else both
    for name in ("first", "sentence"):
        r32 = P.verdict(ref32[name].astype(np.float32), ref[name])
        got = run(api, tmp_path, blob, x, name="text", select="#" + name)
        rk = P.verdict(got, ref[name])
        print(f"\ntext encoder {cfg} x{scale} {kw} {name}: numpy-f32 {r32:.4f} kernel {rk:.4f}")
        assert r32 <= 0.25, (name, r32)
        assert rk <= 1.0, (name, rk)


def test_text_encoder_left_padded(api, tmp_path):
    """padding on the left: the first step is a padded QUERY there (still computed, as ONNX defines it), the sentence head ignores it"""
    cfg = ENCODERS[0][0]
    spec = W.text_encoder_spec(**cfg)
    ids, keep, both, _ = W.text_encoder_inputs(spec, encoder_lengths(cfg["T"], 64), seed=2, left=True)
    ref = W.text_encoder_reference(spec, ids, keep)
    blob = W.text_encoder_from_spec(spec)
    for name in ("first", "sentence"):
        assert P.verdict(run(api, tmp_path, blob, both, name="left", select="#" + name), ref[name]) <= 1.0, name


def test_bits_independent_of_call_path(api, tmp_path):
    cfg = ENCODERS[0][0]
    T = cfg["T"]
    spec = W.text_encoder_spec(outputs=2, **cfg)
    rows = 2048 + 333
    ids, keep, flat, _ = W.text_encoder_inputs(spec, encoder_lengths(T, rows, seed=3), seed=3)
    api.load_model("paths", W.write(str(tmp_path / "paths.onnx"), W.text_encoder_from_spec(spec)) + "#sentence")
    try:
        ref = api.predict("paths", flat)
        sub = slice(0, 300)
        assert P.verdict(ref[sub], W.text_encoder_reference(spec, ids[sub], keep[sub])["sentence"]) <= 1.0
        for n in (1, 17, 333, 2048):  # a row's result depends neither on the chunk nor on its neighbours
            assert np.array_equal(api.predict("paths", np.ascontiguousarray(flat[:n])), ref[:n]), n
        assert np.array_equal(api.predict("paths", np.ascontiguousarray(flat[1000:1017])), ref[1000:1017])
        perm = np.random.default_rng(4).permutation(rows)  # other neighbours, other masks around every row
        assert np.array_equal(api.predict("paths", np.ascontiguousarray(flat[perm])), ref[perm])
        cols = [np.ascontiguousarray(flat[:, j]) for j in range(2 * T)]
        assert np.array_equal(api.predict_columns("paths", cols), ref)  # column-major staged chunks == row-major
        api.register_host_memory(flat)
        try:
            assert np.array_equal(api.predict("paths", flat), ref)  # zero-copy == staged
        finally:
            api.unregister_host_memory(flat)
        dev = api.device_ordinal(0)
        d_in, d_out = api.DeviceBuffer(dev, flat.nbytes), api.DeviceBuffer(dev, ref.nbytes)
        d_in.upload(flat)
        api.predict_device("paths", d_in, flat.shape[0], 2 * T, d_out)
        assert np.array_equal(d_out.download(ref.shape), ref)
        outs, errs = [None] * 16, []

        def call(i):
            try:
                outs[i] = api.predict("paths", flat[: 500 + 37 * i])
            except Exception as e:  # noqa: BLE001
                errs.append(e)

        ts = [threading.Thread(target=call, args=(i,)) for i in range(16)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not errs, errs
        for i in range(16):
            assert np.array_equal(outs[i], ref[: 500 + 37 * i]), i
    finally:
        api.unload_model("paths")


def test_sql_surface(api, tmp_path):
    """tok_* and mask_* columns of a table into infera_predict_array, the way tests/test_sql_surface.py drives the extension"""
    from infera_amd import sqlharness as S

    S.lib()
    cfg = ENCODERS[0][0]
    T = cfg["T"]
    spec = W.text_encoder_spec(**cfg)
    ids, keep, flat, _ = W.text_encoder_inputs(spec, encoder_lengths(T, 300), seed=5)
    path = W.write(str(tmp_path / "sql_text.onnx"), W.text_encoder_from_spec(spec))
    S.sql("infera_load_model", "sql_text", path + "#sentence")
    try:
        tok = [np.ascontiguousarray(ids[:, j]).astype(np.int64) for j in range(T)]
        msk = [np.ascontiguousarray(keep[:, j]).astype(np.int32) for j in range(T)]
        got = np.stack(S.sql("infera_predict_array", "sql_text", *tok, *msk))
        assert np.array_equal(got, api.predict("sql_text", flat))
        assert P.verdict(got, W.text_encoder_reference(spec, ids, keep)["sentence"]) <= 1.0
    finally:
        S.sql("infera_unload_model", "sql_text")
