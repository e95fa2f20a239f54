"""bench.py --dump-outputs on CPU tensors: which pairs are written, in which dtypes, within the size limit, and that the runs
written are the sampled pairs' own (the GPU run of the same is tests/test_gpu_scale.py::test_bench_plain_run_dumps_its_last_step)."""
import os

import numpy as np
import torch

import bench


def _step_outputs(n, seed):
    """A step's outputs as bench.py holds them: edit distances, run counts and the dense runs, pair after pair, with every run
    of pair q set to (q % 251, run index % 256) so that a run can be traced back to its pair."""
    rng = np.random.default_rng(seed)
    cnt = rng.integers(0, 40, n)
    ed = rng.integers(0, 5000, n)
    q = np.repeat(np.arange(n), cnt)
    k = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    dense = np.stack([q % 251, k % 256], axis=1).astype(np.uint8).reshape(-1)
    return (torch.from_numpy(ed), torch.from_numpy(cnt.astype(np.int32)), torch.from_numpy(np.concatenate([dense, np.zeros(16, np.uint8)])),
            ed, cnt)


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_dump_writes_every_pair_and_a_seeded_run_sample(tmp_path):
    ed_t, cnt_t, dense_t, ed, cnt = _step_outputs(5000, 1)
    bench.dump_outputs(str(tmp_path / "a"), ed_t, cnt_t, dense_t, 42)
    f = _load(str(tmp_path / "a"))
    assert sorted(f) == ["edit_distance", "pairs", "run_count", "run_pairs", "runs"]
    assert all(a.dtype == np.float64 for k, a in f.items() if k != "runs") and f["runs"].dtype == np.float32
    assert np.array_equal(f["pairs"], np.arange(5000)) and np.array_equal(f["edit_distance"], ed) and np.array_equal(f["run_count"], cnt)
    rp = f["run_pairs"].astype(np.int64)
    assert len(rp) == bench.DUMP_RUN_PAIRS and np.all(np.diff(rp) > 0)
    want = np.concatenate([np.stack([np.full(cnt[q], q % 251), np.arange(cnt[q]) % 256], axis=1) for q in rp])
    assert np.array_equal(f["runs"], want.astype(np.float32))
    # the same step, the same seed: the same files; another seed samples other pairs
    bench.dump_outputs(str(tmp_path / "b"), ed_t, cnt_t, dense_t, 42)
    assert all(np.array_equal(a, _load(str(tmp_path / "b"))[k]) for k, a in f.items())
    bench.dump_outputs(str(tmp_path / "c"), ed_t, cnt_t, dense_t, 43)
    assert not np.array_equal(_load(str(tmp_path / "c"))["run_pairs"], f["run_pairs"])


def test_dump_of_a_large_step_is_sampled_within_64_mb(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_PAIRS", 1000)
    monkeypatch.setattr(bench, "DUMP_RUN_BYTES", 2000 * 8)
    ed_t, cnt_t, dense_t, ed, cnt = _step_outputs(5000, 2)
    bench.dump_outputs(str(tmp_path), ed_t, cnt_t, dense_t, 7)
    f = _load(str(tmp_path))
    p = f["pairs"].astype(np.int64)
    assert len(p) == 1000 and np.all(np.diff(p) > 0)
    assert np.array_equal(f["edit_distance"], ed[p]) and np.array_equal(f["run_count"], cnt[p])
    rp = f["run_pairs"].astype(np.int64)
    assert 0 < len(rp) < bench.DUMP_RUN_PAIRS and len(f["runs"]) == cnt[rp].sum() <= 2000
    assert sum(os.path.getsize(os.path.join(str(tmp_path), x)) for x in os.listdir(str(tmp_path))) < 64 << 20
    # at the real limits the largest dump stays under 64 MB
    assert (3 * 8 * bench.DUMP_MAX_PAIRS + 8 * bench.DUMP_RUN_PAIRS + bench.DUMP_RUN_BYTES) < 64 << 20
