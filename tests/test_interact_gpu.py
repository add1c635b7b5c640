"""The Interact step on the GPU (INTEGRATION.md 2.6 "Feature interactions"): on integer-valued windows every form of the
pairwise dot products and the bi-interaction term has one right answer and the kernel gives its bits at every tile and quad edge; on generic
data every output is within tests/interact_ref.py's bound of float64 and a NaN stays in its row; DLRM's pass-through columns are bit copies
of the bottom MLP's result; the bits do not depend on the call path; and a torch DLRM and a torch DeepFM meet the project's bar.

Whole models, torch float32 against float64 on the same rows (CPU; the suite's fair-case rule wants at most 0.25 of the bar, else the
Linear weights are scaled by 0.25):
    DLRM, 8 tables d = 16, 13 dense columns, bottom 13 -> 64 -> 16, 36 pairs, top 52 -> 64 -> 1, 333 rows, default initialisation   0.0659
    DeepFM, 10 fields d = 8, deep MLP 80 -> 32 -> 1, 333 rows, table initialised N(0, 0.25^2), Linear layers at their defaults      0.0677
Both are fair as initialised, so both run unscaled.  The DeepFM module initialises its embedding table with a standard deviation of 0.25,
not nn.Embedding's 1: DeepFM implementations start their tables small, and with N(0, 1) values the second-order term is a difference of
sums of about 50 that cancels to 0.04 in the worst of these rows, where torch float32 itself stands at 0.4778 of the bar (0.2997 with the
Linear layers scaled by 0.25: the rule's scaling does not reach the term that loses the digits).
"""
import copy

import numpy as np
import pytest

import interact_ref as R
from infera_amd import onnx_writer as W

try:  # (only the whole-model tests need torch)
    import torch
except ImportError:
    torch = None
pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 1e-6  # the bar of tests/test_transformer_gpu.py
ROWS = R.ROWS
BOUNDED = [(3, 4), (16, 5), (17, 16), (27, 16), (33, 18)]  # (k, d): the cases tests/test_interact_ref.py holds float32 numpy to


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
    def __init__(self, api, tmp_path, blob, name="ia", select=""):
        self.api, self.name = api, name
        api.load_model(name, W.write(str(tmp_path / f"{name}.onnx"), blob) + select)

    def __call__(self, x):
        x = np.ascontiguousarray(x, np.float32)
        return self.api.predict(self.name, x.reshape(len(x), -1))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.api.unload_model(self.name)


_exact = {}


def exact_case(k, d):
    """the integer window of ROWS[-1] rows and its Gram matrices, once per (k, d): integers in float64 are exact, so this is the int64 result"""
    if (k, d) not in _exact:
        _exact.clear()  # (one case at a time: the largest holds 2049 x 64 x 130 values)
        t = R.exact_window(ROWS[-1], k, d, seed=k * 1000 + d)
        t64 = t.astype(np.float64)
        z = np.matmul(t64, t64.transpose(0, 2, 1))
        assert np.abs(z).max() < 2 ** 24
        _exact[(k, d)] = (t, z.astype(np.float32).reshape(len(t), -1))
    return _exact[(k, d)]


# ---- exact cases ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", R.KS)
def test_dot_is_exact(api, tmp_path, k):
    """every d at this k, forms 1, 2 and 3, the three selections, all row counts: same bits as the integer result"""
    sels = R.selections(k)
    for d in R.DS:
        t, z = exact_case(k, d)
        models = [("matrix", None, np.arange(k * k)), ("flat", None, np.arange(k * k))]
        models += [("gather", s, s) for s in sels.values()]
        models += [("index", s % (k * k), s % (k * k)) for s in sels.values()]  # (the exporter's form takes no negative index)
        models.append(("index_folded", sels["triangle"], sels["triangle"]))
        for form, sel, cols in models:
            if len(cols) == 0:  # (k = 1 has no pairs; not among KS)
                continue
            with Served(api, tmp_path, W.interact_dot_model(k, d, form, sel, flatten="reshape" if d % 2 else "flatten")) as m:
                step = [s for s in api.get_plan(m.name)["plan"]["steps"] if s["kind"] == "Interact"]
                assert len(step) == 1 and (step[0]["k"], step[0]["d"], step[0]["P"]) == (k, d, len(cols))
                for rows in ROWS:
                    got = m(t[:rows])
                    assert got.reshape(rows, -1).shape == (rows, len(cols)) and same_bits(got, z[:rows][:, cols]), (k, d, form, rows)


@pytest.mark.parametrize("source", ["embed", "concat"])
def test_dot_is_exact_behind_an_embed_window_and_a_concat(api, tmp_path, source):
    k, d = 17, 5
    table = R.exact_window(1, 40, d, seed=3)[0]
    sel = R.selections(k)["mixed"]
    rng = np.random.default_rng(8)
    with Served(api, tmp_path, W.interact_dot_model(k, d, "gather", sel, source, table)) as m:
        for rows in ROWS:
            if source == "embed":
                ids = rng.integers(0, 40, (rows, k))
                t, x = table[ids], ids.astype(np.float32)
            else:
                t = R.exact_window(rows, k, d, seed=rows)
                x = t
            t64 = t.astype(np.float64)
            want = np.matmul(t64, t64.transpose(0, 2, 1)).reshape(rows, -1)[:, sel]
            assert same_bits(m(x), want), (source, rows)


@pytest.mark.parametrize("k", R.KS)
def test_fm_is_exact(api, tmp_path, k):
    for d in R.DS:
        t, _ = exact_case(k, d)
        cases = [dict(), dict(square="pow", h=0.5, h_side="left")]
        if R.exact_fm_ok(k, d, True):
            cases += [dict(h=0.5, sum_last=True), dict(h=0.5, sum_last=True, h_after=True, keepdims=1)]
        for kw in cases:
            want = R.fm_reference(t, kw.get("h"), kw.get("sum_last", False))
            assert np.abs(want).max() < 2 ** 24
            with Served(api, tmp_path, W.interact_fm_model(k, d, **kw)) as m:
                for rows in ROWS:
                    assert same_bits(m(t[:rows]), want[:rows]), (k, d, kw, rows)


# ---- bounded cases ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,d", BOUNDED)
def test_generic_data_within_the_bound(api, tmp_path, k, d):
    """standard normal values, one row scaled by 1e18 and one by 1e-18: every output within the derived bound of float64, the worst share
    printed; a NaN placed in one row changes that row only"""
    rows = 301
    t = R.normal_window(rows, k, d, seed=k + d)  # (the window tests/test_interact_ref.py checks in float32 numpy is its first 65 rows' twin)
    sel = R.selections(k)["mixed"]
    poisoned = t.copy()
    poisoned[7, k // 2, d // 2] = np.nan
    runs = [("dot matrix", W.interact_dot_model(k, d, "matrix"), R.dot_reference(t), R.dot_bound(t)),
            ("dot gather", W.interact_dot_model(k, d, "gather", sel), R.dot_reference(t, sel), R.dot_bound(t, sel))]
    for h, sum_last, after in ((None, False, False), (0.5, False, False), (0.5, True, False), (0.5, True, True)):
        runs.append((f"fm h={h} sum={sum_last} after={after}", W.interact_fm_model(k, d, h=h, sum_last=sum_last, h_after=after), R.fm_reference(t, h, sum_last),
                     R.fm_bound(t, h, sum_last)))
    for what, blob, ref, bound in runs:
        with Served(api, tmp_path, blob) as m:
            got = m(t)
            print(f"\nk={k} d={d} {what}: worst error / bound {R.worst_over_bound(got, ref, bound):.3f}")
            assert R.within(got, ref, bound), (what, R.worst_over_bound(got, ref, bound))
            bad = m(poisoned)
            assert np.isnan(bad[7]).any(), what
            assert same_bits(np.delete(bad, 7, axis=0), np.delete(got, 7, axis=0)), what


def test_fm_over_scalar_fields_keeps_its_operators_and_its_values(api, tmp_path):
    """(sum x)^2 - sum x^2 on a rank-2 [N, k] activation is not the step's: the single operators serve it as they always did"""
    x = np.random.default_rng(2).standard_normal((301, 6)).astype(np.float32)
    nodes, inits = [], []
    cur, _ = W.interact_fm_nodes(nodes, inits, "X", 1, keepdims=1, h=0.5)
    with Served(api, tmp_path, W.model("scalar_fm", nodes, inits, [W.value_info("X", ["N", 6])], [W.value_info(cur, ["N", 1])])) as m:
        assert [s["kind"] for s in api.get_plan(m.name)["plan"]["steps"]].count("Interact") == 0
        x64 = x.astype(np.float64)
        want = 0.5 * (x64.sum(axis=1, keepdims=True) ** 2 - (x64 * x64).sum(axis=1, keepdims=True))
        # the bound of the window formula with the 6 scalars as fields of d = 1
        t = x[:, :, None]
        assert R.within(m(x), want, R.fm_bound(t, 0.5))


# ---- DLRM's pass-through ----------------------------------------------------------------------------------------------------------------
def dlrm_inputs(spec, rows, seed):
    rng = np.random.default_rng(seed)
    x_cat = np.stack([rng.integers(0, v, rows) for v in spec["cards"]], axis=1)
    x_num = rng.standard_normal((rows, spec["numeric"])).astype(np.float32)
    return x_cat, x_num, np.ascontiguousarray(np.concatenate([x_cat.astype(np.float32), x_num], axis=1))


@pytest.mark.parametrize("form", ["gather", "index"])
def test_pass_through_columns_are_the_bottom_mlps_bits(api, tmp_path, form):
    spec = W.dlrm_spec(cards=(7, 300, 5, 1000, 11), d=5, numeric=4, bottom=(16,), top=(16,), seed=3)
    blob = W.dlrm_from_spec(spec, extra_outputs=True, form=form)
    with Served(api, tmp_path, blob, "r", "#R") as r, Served(api, tmp_path, blob, "xb", "#xb") as xb:
        step = [s for s in api.get_plan("r")["plan"]["steps"] if s["kind"] == "Interact"]
        assert len(step) == 1 and step[0]["pass_through"] == [{"src": 0, "len": 5, "out": 0}] and step[0]["out_cols"] == 5 + 15
        assert api.get_plan("r")["plan"]["steps"][-1]["kind"] == "Interact"  # the Concat is the step: nothing copies behind it
        for rows in ROWS:
            x_cat, x_num, x = dlrm_inputs(spec, rows, seed=rows)
            got, bottom = r(x), xb(x)
            assert got.shape == (rows, 20) and same_bits(got[:, :5], bottom), rows
            ref = W.dlrm_reference(spec, x_cat, x_num)
            t = ref["T"].astype(np.float32)  # (the kernel's T holds the f32 bottom result; close enough for the bound's magnitudes)
            t[:, 0] = bottom
            assert R.within(got[:, 5:], R.dot_reference(t, spec["sel"]), R.dot_bound(t, spec["sel"])), rows


# ---- call paths -------------------------------------------------------------------------------------------------------------------------
def test_bits_independent_of_call_path(api, tmp_path):
    spec = W.dlrm_spec(cards=(7, 300, 5, 1000), d=8, numeric=3, bottom=(16,), top=(16, 4), seed=5)
    rows = 2048
    x_cat, x_num, x = dlrm_inputs(spec, rows + 333, seed=9)
    with Served(api, tmp_path, W.dlrm_from_spec(spec), name="paths") as m:
        ref = m(x)
        assert worst_ratio(ref, W.dlrm_reference(spec, x_cat, x_num)["output"]) <= 1.0
        for n in (1, 17, 333, 2048):  # a chunk prefix: a row's result does not depend on its neighbours
            assert np.array_equal(m(x[:n]), ref[:n]), n
        assert np.array_equal(m(x[1000:1017]), ref[1000:1017])  # a slice from the middle
        cols = [np.ascontiguousarray(x_cat[:, j]) for j in range(4)] + [np.ascontiguousarray(x_num[:, j]) for j in range(3)]  # int64 and f32 columns
        assert np.array_equal(api.predict_columns("paths", cols), ref)
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
    # the window as the model input itself (the step reads the call's rows where they lie), both modes
    t = R.normal_window(rows + 333, 27, 16, seed=1)
    flat = np.ascontiguousarray(t.reshape(len(t), -1))
    for blob in (W.interact_dot_model(27, 16, "gather", R.selections(27)["triangle"]), W.interact_fm_model(27, 16, h=0.5, sum_last=True)):
        with Served(api, tmp_path, blob, name="direct") as m:
            ref = m(flat)
            for n in (1, 17, 333, 2048):
                assert np.array_equal(m(flat[:n]), ref[:n]), n
            assert np.array_equal(m(flat[1000:1017]), ref[1000:1017])
            api.register_host_memory(flat)
            try:
                assert np.array_equal(api.predict("direct", flat), ref)
            finally:
                api.unregister_host_memory(flat)
            dev = api.device_ordinal(0)
            d_in, d_out = api.DeviceBuffer(dev, flat.nbytes), api.DeviceBuffer(dev, ref.nbytes)
            d_in.upload(flat)
            api.predict_device("direct", d_in, flat.shape[0], flat.shape[1], d_out)
            assert np.array_equal(d_out.download(ref.shape), ref)


# ---- whole models at the project's bar --------------------------------------------------------------------------------------------------
DLRM_CARDS, DLRM_D, DLRM_DENSE = (10, 100, 1000, 50, 7, 3, 20, 64), 16, 13
DEEPFM_CARDS, DEEPFM_D = (10, 100, 1000, 50, 7, 3, 20, 64, 5, 30), 8


def torch_dlrm():
    class Dlrm(torch.nn.Module):
        def __init__(self):
            super().__init__()
            k = len(DLRM_CARDS) + 1
            self.embs = torch.nn.ModuleList([torch.nn.Embedding(v, DLRM_D) for v in DLRM_CARDS])
            self.bot = torch.nn.ModuleList([torch.nn.Linear(DLRM_DENSE, 64), torch.nn.Linear(64, DLRM_D)])
            self.top = torch.nn.ModuleList([torch.nn.Linear(DLRM_D + k * (k - 1) // 2, 64), torch.nn.Linear(64, 1)])
            self.li = torch.tensor([i for i in range(k) for j in range(i)])
            self.lj = torch.tensor([j for i in range(k) for j in range(i)])

        def forward(self, x_cat, x_num):
            x = x_num
            for lin in self.bot:
                x = torch.relu(lin(x))
            ly = [e(x_cat[:, j]) for j, e in enumerate(self.embs)]
            T = torch.cat([x] + ly, dim=1).view(x.shape[0], -1, DLRM_D)
            Z = torch.bmm(T, torch.transpose(T, 1, 2))
            R_ = torch.cat([x, Z[:, self.li, self.lj]], dim=1)
            return self.top[1](torch.relu(self.top[0](R_)))

    return Dlrm().eval()


def torch_deepfm():
    class DeepFM(torch.nn.Module):
        def __init__(self):
            super().__init__()
            V, k = sum(DEEPFM_CARDS), len(DEEPFM_CARDS)
            self.emb, self.first = torch.nn.Embedding(V, DEEPFM_D), torch.nn.Embedding(V, 1)
            torch.nn.init.normal_(self.emb.weight, std=0.25)  # (a small-variance table, as DeepFM implementations initialise it: the module docstring)
            self.deep = torch.nn.ModuleList([torch.nn.Linear(k * DEEPFM_D, 32), torch.nn.Linear(32, 1)])
            self.off = torch.tensor(np.concatenate([[0], np.cumsum(DEEPFM_CARDS)[:-1]]))

        def forward(self, x_cat):
            idx = x_cat + self.off
            v = self.emb(idx)
            y1 = self.first(idx).flatten(1).sum(dim=1, keepdim=True)
            s = v.sum(dim=1)
            y2 = 0.5 * (s * s - (v * v).sum(dim=1)).sum(dim=1, keepdim=True)
            return y1 + y2 + self.deep[1](torch.relu(self.deep[0](v.flatten(1))))

    return DeepFM().eval()


def torch_cases(which):
    """(float64 result, float32 result, writer spec, the call's f32 table, the index columns) of the torch model"""
    rng = np.random.default_rng(3)
    lin = lambda m: (m.weight.detach().numpy().astype(np.float32).T.copy(), m.bias.detach().numpy().astype(np.float32).copy())  # noqa: E731
    if which == "dlrm":
        torch.manual_seed(5)
        net = torch_dlrm()
        x_cat = np.stack([rng.integers(0, v, 333) for v in DLRM_CARDS], axis=1)
        x_num = rng.standard_normal((333, DLRM_DENSE)).astype(np.float32)
        with torch.no_grad():
            ref = copy.deepcopy(net).double()(torch.from_numpy(x_cat), torch.from_numpy(x_num).double()).numpy()
            ref32 = net(torch.from_numpy(x_cat), torch.from_numpy(x_num)).double().numpy()
        spec = W.from_torch_dlrm(list(net.embs), list(net.bot), list(net.top))
        return ref, ref32, spec, np.concatenate([x_cat.astype(np.float32), x_num], axis=1), (x_cat, x_num)
    torch.manual_seed(9)
    net = torch_deepfm()
    x_cat = np.stack([rng.integers(0, v, 333) for v in DEEPFM_CARDS], axis=1)
    with torch.no_grad():
        ref = copy.deepcopy(net).double()(torch.from_numpy(x_cat)).numpy()
        ref32 = net(torch.from_numpy(x_cat)).double().numpy()
    spec = {"cards": list(DEEPFM_CARDS), "d": DEEPFM_D, "table": net.emb.weight.detach().numpy().astype(np.float32).copy(),
            "first": net.first.weight.detach().numpy().astype(np.float32).copy(), "offsets": net.off.numpy().astype(np.int64), "mlp": [lin(m) for m in net.deep]}
    return ref, ref32, spec, x_cat.astype(np.float32), (x_cat,)


@pytest.mark.skipif(torch is None, reason="needs torch")
def test_dlrm_from_torch(api, tmp_path):
    ref, ref32, spec, x, (x_cat, x_num) = torch_cases("dlrm")
    r32 = worst_ratio(ref32, ref)
    with Served(api, tmp_path, W.dlrm_from_spec(spec), name="dlrm") as m:
        steps = api.get_plan("dlrm")["plan"]["steps"]
        ia = [s for s in steps if s["kind"] == "Interact"]
        assert len(ia) == 1 and (ia[0]["k"], ia[0]["d"], ia[0]["P"], ia[0]["out_cols"], ia[0]["tile"]) == (9, 16, 36, 52, 16)
        assert ia[0]["pass_through"] == [{"src": 0, "len": 16, "out": 0}] and [s["kind"] for s in steps].count("Embed") == 1
        got = m(x)
    rk = worst_ratio(got, ref)
    print(f"\nDLRM: torch-f32 {r32:.4f} kernel {rk:.4f}")
    assert r32 <= 0.25, r32
    assert rk <= 1.0, rk
    assert worst_ratio(W.dlrm_reference(spec, x_cat, x_num)["output"], ref) <= 0.01  # the numpy restatement is the same function


@pytest.mark.skipif(torch is None, reason="needs torch")
def test_deepfm_from_torch(api, tmp_path):
    ref, ref32, spec, x, (x_cat,) = torch_cases("deepfm")
    r32 = worst_ratio(ref32, ref)
    with Served(api, tmp_path, W.deepfm_from_spec(spec), name="deepfm") as m:
        steps = api.get_plan("deepfm")["plan"]["steps"]
        ia = [s for s in steps if s["kind"] == "Interact"]
        assert len(ia) == 1 and (ia[0]["mode"], ia[0]["k"], ia[0]["d"], ia[0]["sum_last"], ia[0]["h"]) == ("fm", 10, 8, True, 0.5)
        got = m(x)
    rk = worst_ratio(got, ref)
    print(f"\nDeepFM: torch-f32 {r32:.4f} kernel {rk:.4f}")
    assert r32 <= 0.25, r32
    assert rk <= 1.0, rk
    assert worst_ratio(W.deepfm_reference(spec, x_cat)["output"], ref) <= 0.01
