"""bench.py's options and its output dump, without a GPU: a plain run is the default, --steps is the number of timed
steps, and --dump-outputs writes float32 / float64 arrays, a fixed sample of the queries when the batch is too large."""
import os

import numpy as np
import pytest

import bench


def test_plain_run_is_the_default():
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.full, a.steps, a.warmup, a.dump_outputs) == (False, 7, 2, "")
    assert bench.parse_args(["--full"]).full
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])


def test_options_reach_the_worker(tmp_path):
    a = bench.parse_args(["--full", "--dump-outputs", str(tmp_path / "out")])
    argv = bench.passthrough(a)
    assert "--full" in argv
    assert argv[argv.index("--dump-outputs") + 1] == str(tmp_path / "out")
    assert "--dump-outputs" not in bench.passthrough(bench.parse_args([]))


def _batch(nq, ef, seed=0):
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, 1 << 20, (nq, ef)).astype(np.int32)
    ids[:, -1] = -1  # PH_EMPTY32 padding
    return (ids, rng.random((nq, ef), dtype=np.float32), np.full(nq, ef - 1, np.int32),
            rng.integers(0, 1000, (nq, 2)).astype(np.int32), np.zeros(nq, np.int32))


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_whole_batch(tmp_path):
    ids, d, ln, st, status = _batch(500, 64)
    names = bench.dump_outputs(str(tmp_path), ids, d, ln, st, status)
    out = _load(str(tmp_path))
    assert sorted(out) == names == ["distances", "ids", "lengths", "rows", "stats", "status"]
    assert all(a.dtype in (np.float32, np.float64) for a in out.values())
    assert (out["rows"] == np.arange(500)).all()
    assert (out["ids"] == ids.view(np.uint32)).all() and out["ids"][0, -1] == 0xFFFFFFFF
    assert (out["distances"] == d).all() and (out["stats"] == st).all() and (out["lengths"] == ln).all()


def test_dump_of_a_large_batch_is_a_fixed_sample(tmp_path):
    ids, d, ln, st, status = _batch(30000, 256)  # 92 MB as float64 ids + float32 distances
    bench.dump_outputs(str(tmp_path / "a"), ids, d, ln, st, status)
    bench.dump_outputs(str(tmp_path / "b"), ids, d, ln, st, status)
    total = sum(os.path.getsize(os.path.join(str(tmp_path / "a"), f)) for f in os.listdir(str(tmp_path / "a")))
    assert total <= bench.DUMP_BYTES
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    rows = a["rows"].astype(np.int64)
    assert 0 < len(rows) < 30000 and (np.diff(rows) > 0).all()
    assert all((a[k] == b[k]).all() for k in a)
    assert (a["distances"] == d[rows]).all() and (a["ids"] == ids[rows].view(np.uint32)).all()
