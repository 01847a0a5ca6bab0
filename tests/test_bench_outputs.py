"""bench.py --dump-outputs: the files hold the step's outputs exactly, as float32 / float64."""
import numpy as np

import bench


def test_dump_outputs_round_trips_every_output(tmp_path):
    nq, size = 3, 10
    rng = np.random.default_rng(7)
    outs = (rng.random((nq, size), dtype=np.float32),                                   # scores
            rng.integers(0, 2**31 - 1, (nq, size), dtype=np.int32),                      # docs
            rng.integers(0, 8, (nq, size), dtype=np.int32),                              # shard
            np.full(nq, size, np.int32),                                                 # count
            np.array([10_000_000, 2**40 + 1, 0], np.int64),                              # total
            rng.random(nq, dtype=np.float32))                                            # max_score
    d = tmp_path / "out"
    bench.dump_outputs(str(d), outs)
    assert sorted(p.name for p in d.iterdir()) == sorted(n + ".npy" for n in bench.OUTPUT_NAMES)
    for name, want in zip(bench.OUTPUT_NAMES, outs):
        got = np.load(d / (name + ".npy"))
        assert got.dtype == (np.float32 if want.dtype == np.float32 else np.float64)
        assert got.shape == want.shape
        assert np.array_equal(got.astype(want.dtype), want)
        if want.dtype == np.float32:
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert not (d / "rows.npy").exists()


def test_dump_outputs_samples_the_same_queries_beyond_the_cap(tmp_path, monkeypatch):
    nq, size = 64, 4
    outs = (np.arange(nq * size, dtype=np.float32).reshape(nq, size),
            np.arange(nq * size, dtype=np.int32).reshape(nq, size),
            np.zeros((nq, size), np.int32), np.full(nq, size, np.int32),
            np.arange(nq, dtype=np.int64), np.arange(nq, dtype=np.float32))
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 1024)
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), outs)
    rows = np.load(tmp_path / "a" / "rows.npy").astype(np.int64)
    assert 0 < len(rows) < nq and np.all(np.diff(rows) > 0)
    total = 0
    for name, want in zip(bench.OUTPUT_NAMES, outs):
        got = np.load(tmp_path / "a" / (name + ".npy"))
        assert np.array_equal(got, want[rows].astype(got.dtype))
        assert np.array_equal(got, np.load(tmp_path / "b" / (name + ".npy")))   # the same sample every run
        total += got.nbytes
    assert total + rows.nbytes <= 1024
