"""bench.py's --dump-outputs and argument checks, without a GPU: what it writes from a step's packed records, and what it refuses."""
import importlib.util
import os

import numpy as np
import pytest

import libadsb_amd as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _records(n, seed):
    rng = np.random.default_rng(seed)
    rec = np.zeros(n, dtype=A.PACKED_DTYPE)
    for f in A.PACKED_DTYPE.names:
        info = np.iinfo(A.PACKED_DTYPE[f])
        rec[f] = rng.integers(info.min, info.max, n, endpoint=True, dtype=A.PACKED_DTYPE[f])
    return rec


def _dump_bytes(path):
    return sum(os.path.getsize(os.path.join(path, f)) for f in os.listdir(path))


def test_dump_writes_every_record_exactly_in_float64(bench, tmp_path):
    rec = _records(5000, 1)
    info = bench.dump_records(str(tmp_path), rec)
    assert info["records"] == info["written"] == 5000
    assert sorted(os.listdir(tmp_path)) == sorted(["records_index.npy"] + ["records_%s.npy" % f for f in A.PACKED_DTYPE.names])
    assert np.array_equal(np.load(tmp_path / "records_index.npy"), np.arange(5000))
    for f in A.PACKED_DTYPE.names:
        got = np.load(tmp_path / ("records_%s.npy" % f))
        assert got.dtype == np.float64 and np.array_equal(got.astype(A.PACKED_DTYPE[f]), rec[f]), f


def test_dump_of_a_large_step_is_a_fixed_sample_under_the_limit(bench, tmp_path):
    n = 700_000  # 15 files x 8 bytes a record: more than the limit
    rec = _records(n, 2)
    a, b = tmp_path / "a", tmp_path / "b"
    info = bench.dump_records(str(a), rec)
    bench.dump_records(str(b), rec)
    assert info["records"] == n and 0 < info["written"] < n
    assert _dump_bytes(a) <= bench.DUMP_LIMIT_BYTES
    idx = np.load(a / "records_index.npy")
    assert len(idx) == info["written"] and np.all(np.diff(idx) > 0) and idx[-1] < n
    assert np.array_equal(idx, np.load(b / "records_index.npy"))  # the same sample on every run
    for f in A.PACKED_DTYPE.names:
        assert np.array_equal(np.load(a / ("records_%s.npy" % f)), rec[f][idx.astype(np.int64)].astype(np.float64)), f


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--dump-outputs", "d", "--workload", "uat978"], ["--dump-outputs", "d", "--gpus", "2"]])
def test_bench_refuses_what_it_cannot_do(bench, argv):
    with pytest.raises(SystemExit):
        bench.parse_args(argv)


def test_bench_steps_and_dump_arguments(bench):
    args = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2", "--dump-outputs", "d"])
    assert args.steps == 7 and args.warmup == 2 and args.dump_outputs == "d"
