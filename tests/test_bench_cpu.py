"""bench.py --dump-outputs without a GPU: what a run writes is bounded, float32, and the same batch rows in every run."""
import importlib.util
import os
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_samples_fixed_rows_within_budget(tmp_path):
    bench = load_bench()
    rows, n = 300, 32768            # 256 KiB a row, 75 MiB in all: more than DUMP_BYTES
    data = torch.arange(rows, dtype=torch.float32).reshape(rows, 1, 1).expand(rows, n, 2).contiguous()
    wl = types.SimpleNamespace(name="c2c", data=data, torch=torch, tkey="c2c32768")
    got = []
    for run, rank, world in (("a", 0, 1), ("b", 0, 1), ("c", 1, 2)):
        bench.Workload.dump_outputs(wl, str(tmp_path / run), rank, world)
        name = "c2c32768.npy" if world == 1 else "c2c32768_rank%d.npy" % rank
        y = np.load(str(tmp_path / run / name))
        assert y.dtype == np.float32 and y.nbytes <= bench.DUMP_BYTES // world
        assert y.shape == (bench.DUMP_BYTES // world // (n * 8), n, 2)
        picked = y[:, 0, 0].astype(np.int64)
        assert np.all(np.diff(picked) > 0) and picked[-1] < rows
        assert np.array_equal(y, data.numpy()[picked])      # whole rows, as the step left them
        got.append(y)
    assert np.array_equal(got[0], got[1])


def test_dump_outputs_writes_small_outputs_whole(tmp_path):
    bench = load_bench()
    out = torch.rand((8, 1024), generator=torch.Generator().manual_seed(3))
    wl = types.SimpleNamespace(name="pconv", out=out, torch=torch, tkey="pconv1024x94")
    bench.Workload.dump_outputs(wl, str(tmp_path), 0, 1)
    assert np.array_equal(np.load(str(tmp_path / "pconv1024x94.npy")), out.numpy())
