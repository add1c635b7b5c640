"""The Embed step on the GPU: looked-up values are bit copies (np.array_equal with table[idx], with the Concat and as a window), a bad index
fails its own call and nothing else, every call path gives the same bits, and two whole models meet the project's bar against float64
(INTEGRATION.md 2.6 "Embedding lookups").

Whole models, torch float32 against float64 on the same cases (CPU, default initialisation; the suite's fair-case rule wants at most 0.25
of the bar, else the Linear weights are scaled by 0.25):
    entity-embedding MLP (5 tables d = 2, 4, 7, 16, 3 + 6 numeric, 64 -> 32 -> 1), 333 rows       0.0093   (scaled by 0.25: 0.0005)
    shared table + offsets, k = 8, d = 32, 2-layer TransformerEncoder + mean head, 256 rows      0.0405   (scaled by 0.25: 0.0151)
Both are fair at default weights, so both run unscaled."""
import copy
import threading

import numpy as np
import pytest

from infera_amd import onnx_writer as W

try:  # (only the whole-model tests need torch)
    import torch
except ImportError:
    torch = None
pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 1e-6  # the bar of tests/test_transformer_gpu.py
ROWS = (1, 63, 64, 65, 301, 2049)


@pytest.fixture(scope="module")
def api(built):
    from infera_amd import capi

    assert capi.device_count() >= 1, capi.get_devices()
    return capi


def worst_ratio(got, ref):
    got, ref = np.asarray(got, np.float64).reshape(-1), np.asarray(ref, np.float64).reshape(-1)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.max(np.abs(got - ref) / (RTOL * np.abs(ref) + ATOL)))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32).reshape(-1), np.ascontiguousarray(b, np.float32).reshape(-1)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


class Served:
    def __init__(self, api, tmp_path, blob, name="emb"):
        self.api, self.name = api, name
        api.load_model(name, W.write(str(tmp_path / f"{name}.onnx"), blob))

    def __call__(self, x):
        return self.api.predict(self.name, np.ascontiguousarray(x, np.float32))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.api.unload_model(self.name)


def i64(name, v):
    return W.tensor(name, np.asarray(v, dtype=np.int64))


def a_table(V, d, seed=0):
    """every bit pattern matters: normals of both signs, a denormal, zeros of both signs, an infinity and a NaN with a payload"""
    t = np.random.default_rng(seed).standard_normal((V, d)).astype(np.float32)
    flat = t.reshape(-1)
    odd = np.array([0x00000001, 0x80000000, 0x7F800000, 0x7FC01234, 0x00000000], np.uint32).view(np.float32)
    flat[: min(len(flat), len(odd))] = odd[: len(flat)]
    return t


def shared_lookup_model(table, k, m, window=False):
    """k index columns into ONE table ([V, d] or [V]) + m numeric columns.  window: Gather(table, x_cat) -> [N, k, d]; else column j is
    picked, looked up (node 'emb<j>') and everything joined by Concat.  Inputs x_cat [N, k] int64, x_num [N, m]."""
    d = table.shape[1] if table.ndim == 2 else 1
    inputs = [W.value_info("x_cat", ["N", k], W.INT64)] + ([W.value_info("x_num", ["N", m])] if m else [])
    inits = [W.tensor("table", table)]
    if window:
        assert m == 0
        return W.model("win", [W.node("Gather", ["table", "x_cat"], ["Y"], name="emb")], inits, inputs, [W.value_info("Y", ["N", k, d] if table.ndim == 2 else ["N", k])])
    nodes, parts = [], []
    inits.append(i64("ax1", [1]))
    for j in range(k):
        inits.append(i64(f"c{j}", j))
        nodes.append(W.node("Gather", ["x_cat", f"c{j}"], [f"col{j}"], [W.attr_i("axis", 1)], name=f"pick{j}"))
        if table.ndim == 2:
            nodes.append(W.node("Gather", ["table", f"col{j}"], [f"e{j}"], name=f"emb{j}"))
        else:
            nodes.append(W.node("Gather", ["table", f"col{j}"], [f"f{j}"], name=f"emb{j}"))
            nodes.append(W.node("Unsqueeze", [f"f{j}", "ax1"], [f"e{j}"]))
        parts.append(f"e{j}")
    if m:
        parts.append("x_num")
    nodes.append(W.node("Concat", parts, ["Y"], [W.attr_i("axis", 1)], name="join"))
    return W.model("cat", nodes, inits, inputs, [W.value_info("Y", ["N", k * d + m])])


def shared_inputs(V, k, m, rows, seed):
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, V, (rows, k))
    ids[0, 0], ids[-1, -1] = V - 1, 0  # both ends of the table, in the first and the last row
    x_num = rng.standard_normal((rows, m)).astype(np.float32)
    return ids, x_num, np.ascontiguousarray(np.concatenate([ids.astype(np.float32), x_num], axis=1))


def shared_reference(table, ids, x_num):
    t = table.reshape(len(table), -1)
    return np.concatenate([t[ids[:, j]] for j in range(ids.shape[1])] + [x_num], axis=1)


# ---- the lookup alone, bit for bit ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 3, 4, 5, 8, 16, 130])
def test_lookup_with_concat_is_exact(api, tmp_path, d):
    """every (k, V) pair, m stepping through 0 / 1 / 13 so that every k meets every m, all row counts: full and partial tiles, quads inside a piece, across pieces and across
    rows, aligned and unaligned table rows; the window form on the same table"""
    combo = 0
    for V in (1, 2, 1000, 100003):
        table = a_table(V, d, seed=V + d)
        for k in (1, 3, 26):
            m = (0, 1, 13)[(combo + combo // 3) % 3]
            combo += 1
            if V * d > 4_000_000 and k != 3:  # (the 52 MB table once)
                continue
            with Served(api, tmp_path, shared_lookup_model(table, k, m)) as cat, Served(api, tmp_path, shared_lookup_model(table, k, 0, window=True), name="win") as win:
                step = api.get_plan(cat.name)["plan"]["steps"]
                assert [s["kind"] for s in step] == ["Embed"] and step[0]["out_cols"] == k * d + m
                for rows in ROWS:
                    ids, x_num, x = shared_inputs(V, k, m, rows, seed=rows)
                    assert same_bits(cat(x), shared_reference(table, ids, x_num)), (d, V, k, m, rows)
                    got = win(x[:, :k])
                    assert got.shape == (rows, k * d) and same_bits(got, table[ids]), (d, V, k, rows)


def test_pieces_that_straddle_quads(api, tmp_path):
    """d = 3, then d = 4, then one numeric column: rows of 8 floats whose quads lie across pieces, tables whose rows are at no 16-byte
    boundary; and the same pieces in a row of 7 floats (d = 3, d = 4 alone), where no output row is aligned either"""
    for numeric in (1, 0):
        spec = W.embedding_spec(cards=(11, 6), dims=(3, 4), numeric=numeric, hidden=())
        with Served(api, tmp_path, W.embedding_from_spec(spec, "a", tail="none")) as m:
            for rows in ROWS:
                x_cat, x_num, x = W.embedding_inputs(spec, rows, seed=rows)
                assert same_bits(m(x), W.embedding_reference(spec, x_cat, x_num, "a", tail="none")["features"]), (numeric, rows)


def test_rank1_table(api, tmp_path):
    table = a_table(1000, 1, seed=8).reshape(-1)
    for k, m, window in ((1, 0, False), (3, 1, False), (26, 0, True)):
        with Served(api, tmp_path, shared_lookup_model(table, k, m, window=window)) as mdl:
            for rows in ROWS:
                ids, x_num, x = shared_inputs(1000, k, m, rows, seed=rows)
                assert same_bits(mdl(x), shared_reference(table, ids, x_num)), (k, m, rows)


def test_negative_indices_count_from_the_end(api, tmp_path):
    V, d = 37, 5
    table = a_table(V, d, seed=2)
    with Served(api, tmp_path, shared_lookup_model(table, 2, 0)) as m:
        ids = np.stack([np.arange(-V, 0), np.arange(-1, -V - 1, -1)], axis=1)  # all of [-V, -1], both ways
        assert same_bits(m(ids.astype(np.float32)), np.concatenate([table[ids[:, 0] + V], table[ids[:, 1] + V]], axis=1))
        mixed = np.stack([np.arange(-V, V)[: 2 * V], np.arange(V - 1, -V - 1, -1)], axis=1)
        assert same_bits(m(mixed.astype(np.float32)), np.concatenate([table[mixed[:, 0]], table[mixed[:, 1]]], axis=1))


def test_index_values_are_truncated_toward_zero(api, tmp_path):
    V, d = 9, 4
    table = a_table(V, d, seed=3)
    vals = np.array([3.9, -0.5, 0.999, 8.999, -0.999, -1.0, -1.5, -8.99, 2.0000002, 7.5, -9.0, -9.9], np.float32)
    want = np.array([3, 0, 0, 8, 0, -1, -1, -8, 2, 7, -9, -9])
    with Served(api, tmp_path, shared_lookup_model(table, 1, 0)) as m:
        assert same_bits(m(vals.reshape(-1, 1)), table[want])
    # spelling (d): the values of a mixed f32 input behind Cast, and spelling (b): truncated first, then the column's offset
    spec = W.embedding_spec(cards=(9, 12), dims=4, numeric=2, hidden=())
    x = np.array([[3.9, 11.2, 0.5, -1.25], [-0.5, 0.9, np.inf, 3.0], [8.1, -11.9, -0.0, 1e-40]], np.float32)
    with Served(api, tmp_path, W.embedding_from_spec(spec, "d", tail="none")) as m:
        assert same_bits(m(x), W.embedding_reference(spec, x[:, :2], x[:, 2:], "d", tail="none")["features"])
    with Served(api, tmp_path, W.embedding_from_spec(spec, "b", tail="none")) as m:
        pos = np.abs(x)  # (a negative value plus an offset is another column's row: in range, but not this test)
        pos[1, 2] = 1.0
        assert same_bits(m(pos), W.embedding_reference(spec, pos[:, :2], pos[:, 2:], "b", tail="none")["features"])


def test_table_well_beyond_the_l2(api, tmp_path):
    V, d, k = 300_000, 32, 4
    table = np.random.default_rng(1).standard_normal((V, d)).astype(np.float32)
    with Served(api, tmp_path, shared_lookup_model(table, k, 1)) as m:
        ids, x_num, x = shared_inputs(V, k, 1, 2049, seed=6)
        assert same_bits(m(x), shared_reference(table, ids, x_num))


def test_wide_rows(api, tmp_path):
    """the other paths of the kernel: an output row beyond the column -> piece map (40 x 256 = 10240 floats: a search over the pieces,
    one row a work group), the largest LDS layout, and a source row too wide for the LDS tile (9001 columns: indices read where they lie)"""
    table = a_table(30, 256, seed=4)
    with Served(api, tmp_path, shared_lookup_model(table, 40, 0, window=True)) as m:
        assert api.get_plan(m.name)["plan"]["steps"][0]["rows_per_tile"] == 1
        for rows in (1, 65):
            ids, _, x = shared_inputs(30, 40, 0, rows, seed=rows)
            assert same_bits(m(x), table[ids]), rows
    # the most LDS a plan asks for: 1024 pieces (32 KiB of descriptors), the map of an 8192-column row (16 KiB), two source rows of 1024 columns
    table = a_table(77, 8, seed=6)
    with Served(api, tmp_path, shared_lookup_model(table, 1024, 0, window=True)) as m:
        step = api.get_plan(m.name)["plan"]["steps"][0]
        assert (len(step["pieces"]), step["out_cols"], step["rows_per_tile"], step["staged"]) == (1024, 8192, 2, True)
        for rows in (1, 2, 65):
            ids, _, x = shared_inputs(77, 1024, 0, rows, seed=rows)
            assert same_bits(m(x), table[ids]), rows
    t2 = a_table(50, 6, seed=5)
    nodes = [W.node("Gather", ["X", "c0"], ["col"], [W.attr_i("axis", 1)]), W.node("Cast", ["col"], ["ci"], [W.attr_i("to", W.INT64)]), W.node("Gather", ["table", "ci"], ["e"], name="emb"),
             W.node("Slice", ["X", "b", "e_", "ax1"], ["num"], name="numeric"), W.node("Concat", ["e", "num"], ["Y"], [W.attr_i("axis", 1)])]
    inits = [W.tensor("table", t2), i64("c0", 9000), i64("b", [17]), i64("e_", [20]), i64("ax1", [1])]
    with Served(api, tmp_path, W.model("wide", nodes, inits, [W.value_info("X", ["N", 9001])], [W.value_info("Y", ["N", 9])])) as m:
        assert api.get_plan(m.name)["plan"]["steps"][0]["staged"] is False
        for rows in (1, 65, 301):
            x = np.random.default_rng(rows).standard_normal((rows, 9001)).astype(np.float32)
            ids = np.random.default_rng(rows + 1).integers(0, 50, rows)
            x[:, 9000] = ids
            assert same_bits(m(x), np.concatenate([t2[ids], x[:, 17:20]], axis=1)), rows


# ---- bad indices fail their call and nothing else -------------------------------------------------------------------------------------------
BAD_V = 11


@pytest.fixture(scope="module")
def strict_model(api, tmp_path_factory):
    """tables of 7, 11 and 5 rows (d = 3, 4, 2) + 2 numeric columns, spelling (a), no MLP"""
    spec = W.embedding_spec(cards=(7, BAD_V, 5), dims=(3, 4, 2), numeric=2, hidden=())
    api.load_model("strict", W.write(str(tmp_path_factory.mktemp("strict") / "strict.onnx"), W.embedding_from_spec(spec, "a", tail="none")))
    x_cat, x_num, x = W.embedding_inputs(spec, 301, seed=12)
    clean = api.predict("strict", x)
    assert same_bits(clean, W.embedding_reference(spec, x_cat, x_num, "a", tail="none")["features"])
    yield x, clean
    api.unload_model("strict")


@pytest.mark.parametrize("bad", [BAD_V, -BAD_V - 1, np.nan, np.inf, -np.inf, 3e9, 2.0 ** 31], ids=["V", "minus_V_minus_1", "nan", "inf", "minus_inf", "3e9", "2_31"])
@pytest.mark.parametrize("row", [0, 300, 150], ids=["first_row", "last_row", "middle"])
def test_bad_index_fails_the_call_and_names_the_node(api, strict_model, bad, row):
    """The kernel clamps the load to row 0 and raises the call's word: no address is formed from a bad index, so this provokes no fault.
    The one bad value sits in the second of three lookup pieces."""
    x, clean = strict_model
    poisoned = x.copy()
    poisoned[row, 1] = bad
    with pytest.raises(api.InferaError) as e:
        api.predict("strict", poisoned)
    assert str(e.value).endswith("ONNX error: node 'emb1' (Gather): an index is out of range for a table of 11 rows"), str(e.value)
    assert same_bits(api.predict("strict", x), clean)  # the next call on the same model: bit-identical to a clean run
    if row == 150:
        assert same_bits(api.predict("strict", x[140:160]), clean[140:160])


def test_each_piece_reports_its_own_node(api, strict_model):
    x, clean = strict_model
    for col, V in ((0, 7), (2, 5)):
        poisoned = x.copy()
        poisoned[17, col] = V
        with pytest.raises(api.InferaError, match=rf"node 'emb{col}' \(Gather\): an index is out of range for a table of {V} rows"):
            api.predict("strict", poisoned)
    edge = x.copy()
    edge[0, :3], edge[300, :3] = (6, 10, 4), (-7, -11, -5)  # the last valid and the most negative valid index of every table
    api.predict("strict", edge)
    assert same_bits(api.predict("strict", x), clean)


def test_sixteen_callers_one_bad_row(api, strict_model):
    x, clean = strict_model
    outs, errs = [None] * 16, [None] * 16

    def call(i):
        mine = x[: 150 + 9 * i].copy()
        if i == 5:
            mine[77, 1] = BAD_V
        try:
            outs[i] = api.predict("strict", mine)
        except Exception as e:  # noqa: BLE001
            errs[i] = e

    ts = [threading.Thread(target=call, args=(i,)) for i in range(16)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert [i for i in range(16) if errs[i] is not None] == [5], errs
    assert "node 'emb1' (Gather): an index is out of range for a table of 11 rows" in str(errs[5])
    for i in range(16):
        if i != 5:
            assert same_bits(outs[i], clean[: 150 + 9 * i]), i


def test_bad_index_on_the_device_resident_path(api, strict_model):
    x, clean = strict_model
    dev = api.device_ordinal(0)
    d_in, d_out = api.DeviceBuffer(dev, x.nbytes), api.DeviceBuffer(dev, clean.nbytes)
    poisoned = x.copy()
    poisoned[300, 1] = np.nan
    d_in.upload(poisoned)
    with pytest.raises(api.InferaError, match=r"node 'emb1' \(Gather\): an index is out of range for a table of 11 rows"):
        api.predict_device("strict", d_in, 301, x.shape[1], d_out)
    d_in.upload(x)
    api.predict_device("strict", d_in, 301, x.shape[1], d_out)
    assert same_bits(d_out.download(clean.shape), clean)


# ---- a Concat with a computed input, and a lookup with a second reader --------------------------------------------------------------------
def test_scaler_beside_the_lookups_is_exact(api, tmp_path):
    """One Embed step with a gap + the CopyCols of the scaled numeric columns; the scaled columns are (x - offset) * scale, two rounded f32
    operations.  A bad index still names its node."""
    spec = W.embedding_spec(cards=(7, 11, 5), dims=(3, 4, 2), numeric=2, hidden=())
    nodes, inits, _, _, inputs = W.embedding_nodes(spec, "a")
    nodes = [n for n in nodes if b"join" not in n]
    off, sc = np.array([0.5, 1.0], np.float32), np.array([2.0, 4.0], np.float32)
    nodes.append(W.node("Scaler", ["x_num"], ["x_s"], [W.attr_floats("offset", off), W.attr_floats("scale", sc)], name="scale", domain=W.ML_DOMAIN))
    for order in (["e0", "e1", "e2", "x_s"], ["e0", "x_s", "e1", "e2"]):
        blob = W.model("mixed", nodes + [W.node("Concat", order, ["Y"], [W.attr_i("axis", 1)], name="join")], inits, inputs, [W.value_info("Y", ["N", 11])], ml_opset=3)
        with Served(api, tmp_path, blob, name="mixed") as m:
            assert [s["kind"] for s in api.get_plan("mixed")["plan"]["steps"]] == ["SliceCols", "AffineChannel", "Embed", "CopyCols"]
            for rows in ROWS:
                x_cat, x_num, x = W.embedding_inputs(spec, rows, seed=rows)
                parts = {f"e{j}": spec["tables"][j][x_cat[:, j]] for j in range(3)}
                parts["x_s"] = (x_num - off) * sc
                assert same_bits(m(x), np.concatenate([parts[nm] for nm in order], axis=1)), (order, rows)
            x[rows - 1, 2] = 5
            with pytest.raises(api.InferaError, match=r"node 'emb2' \(Gather\): an index is out of range for a table of 5 rows"):
                m(x)


def test_lookup_with_a_second_reader_is_exact(api, tmp_path):
    """Concat(a, b, Relu(a)) with a and b looked up by ONE column: a step of `a` alone for the Relu, the Concat's step with both lookups and a
    gap, one CopyCols; two steps read the input buffer and hold the table of `a`, and either reports a bad index by its own node"""
    ta, tb = a_table(40, 3, seed=1), a_table(25, 2, seed=2)
    nodes = [W.node("Gather", ["x_cat", "c1"], ["col"], [W.attr_i("axis", 1)], name="pick"), W.node("Gather", ["ta", "col"], ["a"], name="emb_a"),
             W.node("Gather", ["tb", "col"], ["b"], name="emb_b"), W.node("Relu", ["a"], ["ar"], name="relu"),
             W.node("Concat", ["a", "b", "ar"], ["Y"], [W.attr_i("axis", 1)], name="join")]
    blob = W.model("second", nodes, [W.tensor("ta", ta), W.tensor("tb", tb), i64("c1", 1)], [W.value_info("x_cat", ["N", 2], W.INT64)], [W.value_info("Y", ["N", 8])])
    with Served(api, tmp_path, blob, name="second") as m:
        assert [s["kind"] for s in api.get_plan("second")["plan"]["steps"]] == ["Embed", "Unary", "Embed", "CopyCols"]
        for rows in ROWS:
            ids = np.random.default_rng(rows).integers(0, 25, (rows, 2))
            want = np.concatenate([ta[ids[:, 1]], tb[ids[:, 1]], np.maximum(ta[ids[:, 1]], np.float32(0))], axis=1)
            got = m(ids.astype(np.float32))
            ok = ~np.isnan(want)  # (the table holds one NaN: what Relu makes of it is the Unary kernel's business)
            assert got.shape == want.shape and same_bits(got[ok], want[ok]) and same_bits(got[:, :5], want[:, :5]), rows
        bad = ids.astype(np.float32)
        bad[0, 1] = 30  # inside table a (40 rows), outside table b (25 rows): only the second lookup of the Concat's step fails
        with pytest.raises(api.InferaError, match=r"node 'emb_b' \(Gather\): an index is out of range for a table of 25 rows"):
            m(bad)
        bad[0, 1] = -41  # outside both: one of the two nodes is named
        with pytest.raises(api.InferaError, match=r"node 'emb_[ab]' \(Gather\): an index is out of range for a table of (40|25) rows"):
            m(bad)
        assert same_bits(m(ids.astype(np.float32))[:, :5], want[:, :5])


# ---- call paths -----------------------------------------------------------------------------------------------------------------------------
def test_bits_independent_of_call_path(api, tmp_path):
    spec = W.embedding_spec(cards=(7, 300, 5, 1000), dims=(3, 4, 2, 7), numeric=3, hidden=(16, 2))
    rows = 2048
    x_cat, x_num, x = W.embedding_inputs(spec, rows + 333, seed=9)
    with Served(api, tmp_path, W.embedding_from_spec(spec, "a"), name="paths") as m:
        ref = m(x)
        assert worst_ratio(ref, W.embedding_reference(spec, x_cat, x_num, "a")["output"]) <= 1.0
        for n in (1, 17, 333, 2048):  # a row's result does not depend on its neighbours
            assert np.array_equal(m(x[:n]), ref[:n]), n
        assert np.array_equal(m(x[1000:1017]), ref[1000:1017])  # a slice from the middle
        cols = [np.ascontiguousarray(x_cat[:, j]) for j in range(4)] + [np.ascontiguousarray(x_num[:, j]) for j in range(3)]  # int64 and f32 columns
        assert np.array_equal(api.predict_columns("paths", cols), ref)  # the column-major staged chunk is handed over row-major
        api.register_host_memory(x)
        try:
            assert np.array_equal(api.predict("paths", x), ref)  # zero-copy == staged
        finally:
            api.unregister_host_memory(x)
        dev = api.device_ordinal(0)
        d_in, d_out = api.DeviceBuffer(dev, x.nbytes), api.DeviceBuffer(dev, ref.nbytes)
        d_in.upload(x)
        api.predict_device("paths", d_in, x.shape[0], x.shape[1], d_out)
        assert np.array_equal(d_out.download(ref.shape), ref)
        bad = x.copy()
        bad[7, 5] = np.nan  # a NaN in a numeric column poisons its own row only
        got = m(bad)
        assert not np.array_equal(got[7], ref[7]) and np.array_equal(np.delete(got, 7, axis=0), np.delete(ref, 7, axis=0))
    spec = W.embedding_spec(cards=(7, 300), dims=(3, 4), numeric=3, hidden=())
    x_cat, x_num, x = W.embedding_inputs(spec, 65, seed=2)
    x[7, 3] = x_num[7, 1] = np.nan
    with Served(api, tmp_path, W.embedding_from_spec(spec, "a", tail="none"), name="nan") as m:  # ... and is itself a copy
        want = W.embedding_reference(spec, x_cat, x_num, "a", tail="none")["features"]
        assert same_bits(m(x), want) and np.isnan(want[7, 8]) and np.isnan(want).sum() == 1


# ---- whole models at the project's bar ------------------------------------------------------------------------------------------------------
def _tabular_net(cards, dims, m, hidden):
    class Tab(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.embs = torch.nn.ModuleList([torch.nn.Embedding(v, d) for v, d in zip(cards, dims)])
            w = [sum(dims) + m] + list(hidden)
            layers = []
            for i, o in zip(w[:-1], w[1:]):
                layers += [torch.nn.Linear(i, o), torch.nn.ReLU()]
            self.fc = torch.nn.Sequential(*layers[:-1])

        def forward(self, x_cat, x_num):
            return self.fc(torch.cat([e(x_cat[:, j]) for j, e in enumerate(self.embs)] + [x_num], dim=1))

    return Tab().eval()


@pytest.mark.skipif(torch is None, reason="needs torch")
def test_entity_embedding_mlp_from_torch(api, tmp_path):
    torch.manual_seed(5)
    cards, dims = (10, 100, 1000, 50, 7), (2, 4, 7, 16, 3)
    net = _tabular_net(cards, dims, 6, (64, 32, 1))
    spec = W.from_torch_tabular(net)
    assert (spec["cards"], spec["dims"], spec["numeric"], [w.shape for w, _ in spec["mlp"]]) == (list(cards), list(dims), 6, [(38, 64), (64, 32), (32, 1)])
    rng = np.random.default_rng(3)
    x_cat = np.stack([rng.integers(0, v, 333) for v in cards], axis=1)
    x_num = rng.standard_normal((333, 6)).astype(np.float32)
    with torch.no_grad():
        ref = copy.deepcopy(net).double()(torch.from_numpy(x_cat), torch.from_numpy(x_num).double()).numpy()
        ref32 = net(torch.from_numpy(x_cat), torch.from_numpy(x_num)).double().numpy()
    r32 = worst_ratio(ref32, ref)
    with Served(api, tmp_path, W.embedding_from_spec(spec, "a"), name="tab") as m:
        plan = api.get_plan("tab")
        # (38 columns into 64 outputs: the lowering pads the row to 40 for the matrix kernels, and the fused chain takes that in: no pass of its own)
        assert [s["kind"] for s in plan["plan"]["steps"]] == ["Embed", "PadCols", "Dense", "Dense", "Dense"]
        assert plan["exec"] == ["normal", "chain_fused", "skipped", "skipped", "skipped"], plan["exec"]
        got = m(np.concatenate([x_cat.astype(np.float32), x_num], axis=1))
    rk = worst_ratio(got, ref)
    print(f"\nentity-embedding MLP: torch-f32 {r32:.4f} kernel {rk:.4f}")
    assert r32 <= 0.25, r32
    assert rk <= 1.0, rk
    assert worst_ratio(W.embedding_reference(spec, x_cat, x_num, "a")["output"], ref) <= 0.01  # the numpy restatement is the same function


@pytest.mark.skipif(torch is None, reason="needs torch")
def test_shared_table_into_a_torch_encoder(api, tmp_path):
    torch.manual_seed(9)
    cards, d = (10, 100, 1000, 50, 7, 3, 20, 64), 32
    emb = torch.nn.Embedding(sum(cards), d)
    layer = torch.nn.TransformerEncoderLayer(d, 4, 64, dropout=0.0, batch_first=True)
    enc = torch.nn.TransformerEncoder(layer, 2, enable_nested_tensor=False).eval()
    head = torch.nn.Linear(d, 1)
    off = torch.tensor(np.concatenate([[0], np.cumsum(cards)[:-1]]))
    x_cat = np.stack([np.random.default_rng(4).integers(0, v, 256) for v in cards], axis=1)

    def run(dtype):
        with torch.no_grad():
            e, c, h = copy.deepcopy(emb).to(dtype), copy.deepcopy(enc).to(dtype), copy.deepcopy(head).to(dtype)
            return h(c(e(torch.from_numpy(x_cat) + off)).mean(dim=1)).double().numpy()

    ref, ref32 = run(torch.float64), run(torch.float32)
    spec = W.embedding_spec(cards=cards, dims=d, numeric=0, hidden=())
    spec["shared"] = emb.weight.detach().numpy().astype(np.float32).copy()
    r32 = worst_ratio(ref32, ref)
    blob = W.embedding_from_spec(spec, "b", tail="encoder", encoder=W.from_torch_encoder(enc, len(cards), head=head), flatten="window")
    with Served(api, tmp_path, blob, name="tok") as m:
        kinds = [s["kind"] for s in api.get_plan("tok")["plan"]["steps"]]
        assert kinds[0] == "Embed" and kinds.count("Embed") == 1 and kinds[-2:] == ["MeanTime", "Dense"] and kinds.count("Attention") == 2
        got = m(x_cat.astype(np.float32))
    rk = worst_ratio(got, ref)
    print(f"\nshared table -> encoder: torch-f32 {r32:.4f} kernel {rk:.4f}")
    assert r32 <= 0.25, r32
    assert rk <= 1.0, rk
