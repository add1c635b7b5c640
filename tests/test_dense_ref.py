"""tests/dense_ref.py checked without a GPU: the float64 restatement against torch's operators in float64, every exact case of
test_dense_exact_gpu.py exact by its own preconditions and reproduced bit for bit by the fp32 oracle (a k-ordered fmaf chain is one of the
summation orders an exact case allows), and every generic case fair: the oracle within half the derived bound.  A case that fails here is
a mistake in the test, found before a GPU is asked."""
from __future__ import annotations

import numpy as np
import pytest

from infera_amd import onnx_writer as W
from tests import dense_ref as R


@pytest.fixture(scope="module")
def O(built):
    from oracle import oracle

    return oracle


def test_table_names_what_the_selection_rule_gives():
    for row, dims in R.TABLE:
        assert R.served_by(dims) == R.expected(row, dims), (row, dims)
    reached = {R.expected(row, dims) for row, dims in R.TABLE}
    assert reached >= {"dense_skinny_kernel", "dense_narrow16g_kernel", "dense_narrow16_kernel", "dense_narrow16s_kernel", "dense_narrow16w_kernel",
                       "dense_narrow_kernel", "chain_fused", "mlp3_fused", "dense_tiled"}
    assert {R.family(257, k, m, aligned=False) for k, m in R.N16S} == {"dense_kernel", "dense_narrow16w_kernel"}  # (K = 256: the wide kernel)
    # dense_kernel<MT>: the rows at which 2, 4 and 8 output tiles per workgroup survive the halving lie far above this suite's
    assert [R.dense_kernel_mt(R.BIG, m) for m in (17, 33, 65, 129, 300)] == [1] * 5 and R.dense_kernel_mt(32768 + 33, 300) == 8


@pytest.mark.parametrize("dims,acts,sm", [((30, 100, 2), None, True), ((128, 256, 64, 1), None, False)], ids=["30x100x2+sm", "128x256x64x1"])
def test_restatement_against_torch_float64(dims, acts, sm):
    import torch

    from oracle import torch_ref

    x = R.generic_inputs(dims[0], 65)["uniform"]
    want = torch_ref.mlp_forward(torch_ref.mlp_layers(dims, torch.float64, seed=77), torch.from_numpy(x).double(), final_softmax=sm).numpy()
    got = R.forward64(R.mlp_weights(dims, seed=77), x, acts, "Softmax" if sm else "")["out"]
    assert got.shape == want.shape and np.abs(got - want).max() <= 1e-13 * max(1.0, np.abs(want).max())


def test_graph_writer_spells_the_same_model(O, tmp_path):
    """gemm / matmul_add / trans_b and onnx_writer.mlp's own graph: one oracle answer"""
    dims = (9, 20, 4)
    layers, x = R.mlp_weights(dims, seed=3), R.generic_inputs(9, 33)["uniform"]
    want = O.Model(W.write(str(tmp_path / "w.onnx"), W.mlp(dims, final_softmax=True, seed=3))).predict(x)
    for form in ("gemm", "matmul_add", "trans_b"):
        got = O.Model(W.write(str(tmp_path / f"{form}.onnx"), R.graph(layers, head="Softmax", form=form))).predict(x)
        assert np.array_equal(got, want), form


@pytest.mark.parametrize("case", R.TABLE, ids=R.case_id)
def test_exact_cases_are_exact_and_the_oracle_reproduces_them(O, tmp_path, case):
    _, dims = case
    rows = R.BIG if R.big_rows(dims) else R.ROWS[-1]
    for kind in R.KINDS:
        layers, x = R.exact_case(kind, dims, rows)
        want = R.assert_exact(layers, x, grid=kind == "grid")
        got = O.Model(W.write(str(tmp_path / f"{kind}.onnx"), R.graph(layers))).predict(x)
        assert np.array_equal(got.reshape(want.shape), want), kind
        if kind == "select":  # every k is read where M >= K, the last column reads the last k
            w = layers[0][0]
            assert (np.count_nonzero(w, axis=0) == 1).all() and w[-1, -1] != 0 and (dims[1] < dims[0] or (np.count_nonzero(w, axis=1) >= 1).all())
        if kind == "onehot":
            assert (np.count_nonzero(x, axis=1) == 1).all()


@pytest.mark.parametrize("case", R.EPILOGUES, ids=lambda c: R.case_id(c) + "-" + c[2])
def test_argmax_cases_tie_on_every_row(O, tmp_path, case):
    _, dims, where = case
    layers, x = R.exact_case("grid", dims, R.BIG if where == "big" else R.ROWS[-1], tie_columns=True)
    R.assert_exact(layers, x, grid=True)
    ref = R.forward64(layers, x, head="ArgMax")
    z = ref["logits"]
    assert ((z == z.max(1, keepdims=True)).sum(1) >= 2).all()
    assert (ref["out"][:, 0] < dims[-1] / 2).all()  # the lower of each pair
    got = O.Model(W.write(str(tmp_path / "a.onnx"), R.graph(layers, head="ArgMax"))).predict(x)
    assert np.array_equal(got.reshape(-1), ref["out"][:, 0].astype(np.float32))


@pytest.mark.parametrize("case", R.GENERIC_DATA, ids=lambda c: "x".join(map(str, c[0])))
def test_generic_cases_are_fair(O, tmp_path, case):
    """the fp32 oracle itself (a sequential fmaf chain) lies within HALF the bound a kernel is held to"""
    dims, acts, sm = case
    layers = R.mlp_weights(dims, seed=31)
    model = O.Model(W.write(str(tmp_path / "g.onnx"), W.mlp(dims, acts=acts, final_softmax=sm, seed=31)))
    for name, x in R.generic_inputs(dims[0]).items():
        ref, bound = R.error_bound(layers, x, acts, "Softmax" if sm else "")
        err = np.abs(model.predict(x).astype(np.float64) - ref)
        assert np.isfinite(bound).all() and (err <= bound / 2).all(), (name, (err / bound).max())
