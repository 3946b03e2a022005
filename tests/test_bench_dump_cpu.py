"""bench.py --dump-outputs without a GPU: dump_outputs() on host tensors -- every row of a small x, the fixed seeded sample of a
large one, and the collection of row shards on rank 0 (a stand-in for torch.distributed's all_gather_object)."""
import importlib.util
import os
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_dump_mod", os.path.join(ROOT, "bench.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b


ST = types.SimpleNamespace(iters=7, converged=0, breakdown=0, half_exit=1, nrm0=3.5, nrm=0.25)


def _load(d):
    return {name: np.load(os.path.join(d, name + ".npy")) for name in ("x", "x_rows", "stats")}


def _x(n):
    return np.random.default_rng(n).standard_normal(n)


def test_every_row_of_a_small_x(bench, tmp_path):
    n = 5000
    x = _x(n)
    bench.dump_outputs(str(tmp_path), torch.from_numpy(x), ST, n, 0, n, 0, 1, None)
    got = _load(str(tmp_path))
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["x_rows"], np.arange(n)) and np.array_equal(got["x"], x)
    assert got["stats"].tolist() == [7, 0, 0, 1, 3.5, 0.25]


def test_a_large_x_is_a_fixed_sample(bench, tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_ROWS", 1000)
    n = 10007
    x = _x(n)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), torch.from_numpy(x), ST, n, 0, n, 0, 1, None)
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    rows = a["x_rows"].astype(np.int64)
    assert len(rows) == 1000 and np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < n
    assert np.array_equal(a["x"], x[rows])
    assert np.array_equal(a["x_rows"], b["x_rows"]) and np.array_equal(a["x"], b["x"])


class _Gather:
    """all_gather_object of `world` ranks: records what every rank contributes, hands out `parts` (when given)"""

    def __init__(self, rank, seen, parts=None):
        self.rank, self.seen, self.parts = rank, seen, parts

    def all_gather_object(self, out, obj):
        self.seen[self.rank] = obj
        for i in range(len(out)):
            out[i] = self.parts[i] if self.parts is not None else np.zeros(0)


@pytest.mark.parametrize("dump_rows", [1000, 1 << 20])
def test_row_shards_are_collected_in_row_order(bench, tmp_path, monkeypatch, dump_rows):
    from cuda_mat_amd.dist import shard_rows
    monkeypatch.setattr(bench, "DUMP_ROWS", dump_rows)
    n, world = 10007, 3
    x = _x(n)
    seen = {}
    for r in range(world):               # what each rank hands to the gather (rank > 0 writes nothing)
        row0, row1, _ = shard_rows(n, world, r)
        d = str(tmp_path / ("rank%d" % r))
        bench.dump_outputs(d, torch.from_numpy(x[row0:row1].copy()), ST, n, row0, row1, r, world, _Gather(r, seen))
        assert os.path.exists(d) == (r == 0)
    row0, row1, _ = shard_rows(n, world, 0)
    d = str(tmp_path / "collected")
    bench.dump_outputs(d, torch.from_numpy(x[row0:row1].copy()), ST, n, row0, row1, 0, world,
                       _Gather(0, {}, [seen[r] for r in range(world)]))
    got = _load(d)
    rows = got["x_rows"].astype(np.int64)
    assert len(rows) == min(n, dump_rows)
    assert np.array_equal(got["x"], x[rows])
