"""The tile queue of the fused MLP's split kernel (mlp_device.inc, mlp3_split_kernel): a wave's first tile is fixed, every later one is claimed
from a head word, and the last wave out zeroes the head and the done count again.  Which wave computes a tile does not enter the arithmetic, so
every launch must equal, BIT FOR BIT, the same rows pushed through infera_predict in chunks of at most 4096 rows -- the tile kernels' path, which
knows no queue.  Row counts sit just above the 32,768 rows below which the tile kernels serve the call; d_out is NaN before every launch, so a
tile nobody claimed shows up."""
import os
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CHUNK = 4096
MODELS = {"c2": (128, 256, 64, 1), "c2x3": (128, 256, 64, 3), "jit": (64, 128, 32, 2)}  # (the third: compiled by hipRTC at load)
SEED = 11


class Env:
    def __init__(self, capi, tmp):
        from infera_amd import onnx_writer

        self.capi = capi
        self.dev = capi.device_ordinal(0)
        self.W = 8 * int(capi.get_devices()["devices"][0]["cus"])  # waves of a full launch: 8 per workgroup, one workgroup per CU
        # rows of each model's table: the longest any test below scans
        self.rows = {"c2": max(200_000, 32 * self.W + 33), "c2x3": 32 * self.W + 33, "jit": 32 * self.W + 33}
        self.d_in, self.x, self.ref = {}, {}, {}
        for name, dims in MODELS.items():
            capi.load_model("tq_" + name, onnx_writer.write(os.path.join(tmp, name + ".onnx"), onnx_writer.mlp(dims)))
            n, k = self.rows[name], dims[0]
            self.d_in[name] = capi.DeviceBuffer(self.dev, n * k * 4)
            capi.synth_fill(self.d_in[name], SEED, 0, n, k)
            self.x[name] = self.d_in[name].download((n, k))
            # the reference, once: chunks of <= 4096 rows through the host ABI (16-row / 32-row tile kernels)
            self.ref[name] = np.concatenate([capi.predict("tq_" + name, self.x[name][r0:r0 + CHUNK]) for r0 in range(0, n, CHUNK)])
            assert self.ref[name].shape == (n, dims[-1]) and not np.isnan(self.ref[name]).any()
            assert capi.get_plan("tq_" + name)["exec"][0] == "mlp3_fused"

    def nan_out(self, name, rows):
        d3 = MODELS[name][-1]
        return self.capi.DeviceBuffer(self.dev, rows * d3 * 4).upload(np.full((rows, d3), np.nan, np.float32))

    def scan(self, name, rows, d_out=None, sync=True):
        d_out = d_out or self.nan_out(name, rows)
        self.capi.predict_device("tq_" + name, self.d_in[name], rows, MODELS[name][0], d_out, sync=sync)
        return d_out

    def check(self, name, rows, d_out):
        got = d_out.download((rows, MODELS[name][-1]))
        bad = np.flatnonzero((got.view(np.uint32) != self.ref[name][:rows].view(np.uint32)).any(axis=1))
        assert bad.size == 0, (name, rows, bad.size, "first bad tile %d" % (bad[0] // 32), "NaN rows %d" % int(np.isnan(got).any(axis=1).sum()))


@pytest.fixture(scope="module")
def env(gpu_api, tmp_path_factory):
    e = Env(gpu_api, str(tmp_path_factory.mktemp("tq")))
    yield e
    for name in MODELS:
        gpu_api.unload_model("tq_" + name)


def test_fewer_tiles_than_waves(env):
    # 1025 tiles, the last of 5 rows; of a full launch's waves (2048 on 256 CUs) about half get no tile at all and still count themselves out
    env.check("c2", 32_773, env.scan("c2", 32_773))


def test_two_tiles_through_the_queue_and_a_ragged_tail(env):
    rows = 32 * env.W + 33  # W first tiles, then two claimed ones: a whole tile and one of a single row
    env.check("c2", rows, env.scan("c2", rows))


def test_about_three_claims_per_wave(env):
    env.check("c2", 200_000, env.scan("c2", 200_000))


def test_back_to_back_launches_leave_the_queue_clean(env):
    # one stream, no synchronisation in between: every launch must find head = done = 0, left by the one before it
    counts = [32_773, 32 * env.W + 33, 40_001, 100_003, 32_773]
    outs = [env.nan_out("c2", n) for n in counts]
    for n, d in zip(counts, outs):
        env.scan("c2", n, d, sync=False)
    env.capi.sync(env.dev)
    for n, d in zip(counts, outs):
        env.check("c2", n, d)


def test_two_threads_have_a_queue_each(env):
    # each thread scans on its own context (its own stream and queue words), both at once over the same model
    errors = []

    def worker(rows):
        try:
            for _ in range(5):
                env.check("c2", rows, env.scan("c2", rows))
        except BaseException as exc:  # noqa: BLE001 -- reported by the asserting thread below
            errors.append(exc)

    threads = [threading.Thread(target=worker, args=(n,)) for n in (70_001, 32 * env.W + 33)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


@pytest.mark.parametrize("name", list(MODELS))
def test_every_row_major_instantiation(env, name):
    for rows in (32_773, 32 * env.W + 33):
        env.check(name, rows, env.scan(name, rows))


@pytest.mark.parametrize("name", ["c2", "c2x3"])
def test_column_major_chunks_above_the_tile_kernels_range(env, name):
    # infera_predict_columns hands a call of up to 24 MiB to the first kernel as ONE column-major chunk: the ahead-of-time XCM kernels
    k = MODELS[name][0]
    for rows in (32_773, 49_001):
        assert 32_768 < rows and rows * k * 4 <= 24 << 20
        got = env.capi.predict_columns("tq_" + name, [np.ascontiguousarray(env.x[name][:rows, c]) for c in range(k)])
        assert got.shape == (rows, MODELS[name][-1])
        assert np.array_equal(got.view(np.uint32), env.ref[name][:rows].view(np.uint32)), (name, rows)
