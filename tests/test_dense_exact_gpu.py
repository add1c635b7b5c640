"""The f32 Dense families (hip/dense.hip), the load-time chain kernel (chain_device.inc) and the fused MLP (mlp_device.inc) against the float64
restatement of tests/dense_ref.py -- not against the fp32 oracle, whose 1e-4 parity bar is some 1,700 roundings wide.

Exact cases: inputs on which a correct fp32 kernel has ONE right answer in any summation order, compared with np.array_equal.  (a) integer
grids: every term counted once -- a duplicated, dropped or neighbouring term moves an integer; (b) signed selections of full-mantissa
activations: +-2^e x_j to the bit, so a kernel that drops low bits of X or of a hidden activation, or reads the wrong k, fails; (c) one-hot
rows against full-mantissa weights: 2^e W[k, m] to the bit.  Every case asserts from the plan what served it (dense_ref.served_by restates
the rule; the plan names the family of a long aligned scan, the run-time family of a short, unaligned or column-major call follows from
dense_ref.family, which the plan cannot report -- there the result alone is asserted and the family printed).

Generic data: every element within the derived bound (dense_ref.error_bound), and the batch's RMS error at most 2 x that of the fp32 oracle's
sequential fmaf chain -- summation order moves an fp32 RMS error by less than sqrt(2), a lost operand part by 2^8 and more.  Measured ratios
(MI355X; profiles/dense_exact_rms_ratios.txt): 0.85 .. 1.12 over the 32 runs -- the dense.hip families 0.97 .. 1.07, the chain kernel
0.91 .. 1.03 (0.85 behind the wide first layer of 130x33x70x9), the fused MLP 1.07 (uniform) and 1.12 (offset); nothing near 1.4."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

from infera_amd import onnx_writer as W
from tests import dense_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SM = {"": 0, "Softmax": 1, "LogSoftmax": 2, "ArgMax": 3}
FUSED_HEAD = {"Softmax": "dense_softmax", "LogSoftmax": "dense_softmax", "ArgMax": "dense_argmax"}


@pytest.fixture(scope="module")
def api(built):
    from infera_amd import capi

    assert capi.device_count() >= 1, capi.get_devices()
    return capi


@pytest.fixture(scope="module")
def O(built):
    from oracle import oracle

    return oracle


class Served:
    """one loaded model and the three ways rows reach it"""

    def __init__(self, api, tmp_path, blob, out_cols):
        self.api, self.out_cols, self.name = api, out_cols, "dense_exact"
        api.load_model(self.name, W.write(str(tmp_path / "m.onnx"), blob))
        self.plan = api.get_plan(self.name)

    def close(self):
        self.api.unload_model(self.name)

    def rows(self, x):
        return self.api.predict(self.name, x).reshape(x.shape[0], self.out_cols)

    def columns(self, x):
        """one column-major chunk"""
        return self.api.predict_columns(self.name, [np.ascontiguousarray(x[:, c]) for c in range(x.shape[1])]).reshape(x.shape[0], self.out_cols)

    def device(self, x, offset=0):
        """a device-resident table in one launch, `offset` bytes past a 16-byte boundary"""
        api, dev = self.api, self.api.device_ordinal(0)
        d_in, d_out = api.DeviceBuffer(dev, x.nbytes + 16), api.DeviceBuffer(dev, x.shape[0] * self.out_cols * 4 + 16)
        try:
            d_in.upload(np.concatenate([np.zeros(offset // 4, np.float32), x.ravel()]))
            r, c = api.predict_device(self.name, d_in, x.shape[0], x.shape[1], d_out, in_offset_bytes=offset)
            assert r * c == x.shape[0] * self.out_cols, (r, c)
            return d_out.download((x.shape[0], self.out_cols))
        finally:
            d_in.free()
            d_out.free()


def check_plan(plan, what, dims, head=""):
    """the plan names `what` for the model's first layer: a fused step's exec kind, or a dense.hip family behind normal / dense_softmax / dense_argmax"""
    ex = plan["exec"][1:] if plan["plan"]["steps"][0]["kind"] == "PadCols" and plan["exec"][0] == "normal" else plan["exec"]  # (a pad pass of its own)
    if what in ("chain_fused", "mlp3_fused", "dense_tiled"):
        assert ex[0] == what, plan["exec"]
        if what == "chain_fused":
            assert plan["chain_kernels"][0].startswith("chain_kernel<" + "x".join(map(str, dims))), plan["chain_kernels"]
        return
    assert ex[0] == (FUSED_HEAD[head] if head else "normal"), plan["exec"]
    assert plan["dense_kernels"][0].startswith(what) and what == R.family(1 << 20, dims[0], dims[1], SM[head]), plan["dense_kernels"]


def colmajor_ok(what, dims):
    return what == "chain_fused" or (len(dims) == 2 and dims[1] <= 16 and dims[0] < 64)  # dense_colmajor_supported / the chain's own reader


@pytest.mark.parametrize("case", R.TABLE, ids=R.case_id)
def test_exact_cases(api, tmp_path, case):
    row, dims = case
    what = R.expected(row, dims)
    K, M = dims[0], dims[-1]
    big = R.big_rows(dims)
    ran = set()
    for kind in R.KINDS:
        layers, x = R.exact_case(kind, dims, R.BIG if big else R.ROWS[-1])
        want = R.assert_exact(layers, x, grid=kind == "grid")
        m = Served(api, tmp_path, R.graph(layers), M)
        try:
            check_plan(m.plan, what, dims)
            single = what.endswith("_kernel")
            for r in R.ROWS:  # plain
                assert np.array_equal(m.rows(x[:r]), want[:r]), (kind, "rows", r)
                ran.add(R.family(r, K, M) if single else what)
            if big:  # one launch above the row threshold: a resident scan (16s; the fused MLP's split kernel), and the host entry (its 32-row tiles)
                assert np.array_equal(m.device(x), want), (kind, "device", R.BIG)
                assert np.array_equal(m.rows(x), want), (kind, "rows", R.BIG)
                ran.add(R.family(R.BIG, K, M) if single else what)
            for r in (33, 257):  # 4 bytes off a 16-byte boundary (the plan cannot report what then runs: the result is asserted, the family printed)
                assert np.array_equal(m.device(x[:r], offset=4), want[:r]), (kind, "unaligned", r)
                ran.add((R.family(r, K, M, aligned=False) if single else what) + " (unaligned)")
            if colmajor_ok(what, dims):
                for r in (33, 257):  # rows & 3 != 0: the chunk's columns start off 16-byte boundaries, no aligned fast path
                    assert np.array_equal(m.columns(x[:r]), want[:r]), (kind, "columns", r)
                    ran.add((R.family(r, K, M, colmajor=True) if single else what) + " (column-major)")
        finally:
            m.close()
    print(f"{R.case_id(case)}: {sorted(ran)}")
    if what.endswith("_kernel"):
        assert what in ran, (what, ran)
    if tuple(dims) in R.N16S and K <= 128:  # the one way dense_kernel is reached at these sizes: 64 / 128-column rows off a 16-byte boundary
        assert "dense_kernel (unaligned)" in ran


@pytest.mark.parametrize("head", ["ArgMax", "Softmax", "LogSoftmax"])
@pytest.mark.parametrize("case", R.EPILOGUES, ids=lambda c: R.case_id(c) + "-" + c[2])
def test_fused_epilogues_on_grids(api, tmp_path, case, head):
    """ArgMax with a tie on every row: the lower index wins.  Softmax / LogSoftmax: their values belong to the bound below; here the ranks -- equal
    scores give equal bits, a larger score never a smaller value, the row's largest value sits at the reference's label."""
    what, dims, where = case
    layers, x = R.exact_case("grid", dims, R.BIG if where == "big" else R.ROWS[-1], tie_columns=True)
    R.assert_exact(layers, x, grid=True)
    ref = R.forward64(layers, x, head="ArgMax")
    z, label = ref["logits"], ref["out"][:, 0].astype(np.float32)
    assert dims[-1] < 2 or ((z == z.max(1, keepdims=True)).sum(1) >= 2).all()
    m = Served(api, tmp_path, R.graph(layers, head=head), 1 if head == "ArgMax" else dims[-1])
    try:
        check_plan(m.plan, R.family(1 << 20, *dims), dims, head)  # exec names the fused form
        runs = {"rows": [(m.rows, r) for r in R.ROWS], "big": [(m.device, R.BIG)], "columns": [(m.columns, 33), (m.columns, 257)]}[where]
        for run, r in runs:
            got = run(x[:r])
            if head == "ArgMax":
                assert np.array_equal(got[:, 0], label[:r]), (where, r)
                continue
            assert np.isfinite(got).all() or head == "LogSoftmax"
            order = np.argsort(z[:r], axis=1, kind="stable")
            zs, gs = np.take_along_axis(z[:r], order, 1), np.take_along_axis(got, order, 1)
            assert (np.diff(gs, axis=1) >= 0).all(), (where, r)
            assert (np.diff(gs, axis=1)[np.diff(zs, axis=1) == 0] == 0).all(), (where, r)
            assert np.array_equal(got[np.arange(r), label[:r].astype(int)], got.max(1))
    finally:
        m.close()


def test_argmax_behind_an_unaligned_pointer_falls_back_to_two_kernels(api, tmp_path):
    """64 -> 10 + ArgMax, rows 4 bytes off a 16-byte boundary: no kernel with the label epilogue reads them (dense_can_fuse_argmax at run time),
    so steps.cpp launches the Dense layer (dense_kernel) and the ArgMax step one after the other -- the plan still names the fused form"""
    dims = (64, 10)
    layers, x = R.exact_case("grid", dims, 257, tie_columns=True)
    label = R.forward64(layers, x, head="ArgMax")["out"].astype(np.float32)
    assert R.family(257, 64, 10, 3, aligned=False) == "" and R.family(257, 64, 10, 0, aligned=False) == "dense_kernel"
    m = Served(api, tmp_path, R.graph(layers, head="ArgMax"), 1)
    try:
        assert m.plan["exec"] == ["dense_argmax", "normal"], m.plan["exec"]
        for r in (33, 257):
            assert np.array_equal(m.device(x[:r], offset=4), label[:r]), r
            assert np.array_equal(m.device(x[:r]), label[:r]), r
    finally:
        m.close()


def test_argmax_is_not_fused_where_the_wide_kernel_is_switched_off(tmp_path):
    """INFERA_DENSE16W=0 (an A/B switch, read once per process): 129 -> 17 + ArgMax has no kernel with the label epilogue left, so the plan must
    not promise one -- dense() used to return without writing"""
    layers, x = R.exact_case("grid", (129, 17), 33, tie_columns=True)
    label = R.forward64(layers, x, head="ArgMax")["out"][:, 0]
    path = W.write(str(tmp_path / "m.onnx"), R.graph(layers, head="ArgMax"))
    np.save(tmp_path / "x.npy", x)
    code = ("import sys, json, numpy as np; sys.path.insert(0, %r); from infera_amd import capi; capi.load_model('m', %r); "
            "y = capi.predict('m', np.load(%r)); print(json.dumps({'exec': capi.get_plan('m')['exec'], 'y': y.reshape(-1).tolist()}))") % (ROOT, path, str(tmp_path / "x.npy"))
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, INFERA_DENSE16W="0"), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res["exec"] == ["normal", "normal"] and res["y"] == label.tolist(), res["exec"]


@pytest.mark.parametrize("case", R.GENERIC_DATA, ids=lambda c: "x".join(map(str, c[0])))
def test_generic_data_within_the_float64_bound(api, O, tmp_path, case):
    dims, acts, sm = case
    layers = R.mlp_weights(dims, seed=31)
    path = W.write(str(tmp_path / "g.onnx"), W.mlp(dims, acts=acts, final_softmax=sm, seed=31))
    oracle = O.Model(path)
    api.load_model("dense_generic", path)
    try:
        plan = api.get_plan("dense_generic")
        for name, x in R.generic_inputs(dims[0]).items():
            ref, bound = R.error_bound(layers, x, acts, "Softmax" if sm else "")
            got = api.predict("dense_generic", x).astype(np.float64)
            err, err_o = np.abs(got - ref), np.abs(oracle.predict(x).astype(np.float64) - ref)
            assert (err_o <= bound / 2).all()  # a fair case
            ratio = R.rms(err) / R.rms(err_o) if R.rms(err_o) > 0 else (np.inf if R.rms(err) > 0 else 0.0)  # (a saturated softmax: both exact)
            print(f"{'x'.join(map(str, dims))} {name}: exec {plan['exec']} {plan.get('dense_kernels', plan.get('chain_kernels', ''))}: "
                  f"worst error / bound = {(err / bound).max():.3f}, RMS error / the oracle's = {ratio:.3f}")
            assert (err <= bound).all(), (name, (err / bound).max())
            assert R.rms(err) <= 2 * R.rms(err_o), (name, ratio)
    finally:
        api.unload_model("dense_generic")
