"""bench.py --dump-outputs on the CPU: which device bytes the dump reads (a fake context stands in for the device), the
seeded sample, the byte budget and the file layout."""
import numpy as np
import pytest

import bench


class FakeDevice:
    """malloc hands out disjoint address ranges; d2h checks bounds and fills float64 rows with their own addresses."""

    def __init__(self):
        self.next, self.allocs, self.reads = 1 << 20, {}, []

    def malloc(self, n):
        p = self.next
        self.next += n + 4096
        self.allocs[p] = n
        return p

    def h2d(self, p, arr):
        pass

    def d2h(self, arr, p):
        assert any(b <= p and p + arr.nbytes <= b + n for b, n in self.allocs.items()), "read out of bounds"
        self.reads.append((p, arr.nbytes))
        arr.reshape(-1)[:] = p + 8 * np.arange(arr.size)


def make_job(lens, batch, C=4, budget=200 << 30):
    lens = np.asarray(lens, np.int64)
    return bench.DspJob(FakeDevice(), None, C, np.zeros(int(lens.sum()), np.int16), lens, batch, "both", 50, 0,
                        out_budget_bytes=budget)


def expected_start(job, u, c):
    """Address of row (utterance u of the shard, channel c): utterances are (C, n) blocks in their batch's output region."""
    first = 0
    for (_, off, nb), ptr in zip(job.batches, job.out_ptr):
        if u < first + nb:
            b = u - first
            n = int(off[b + 1] - off[b])
            return ptr + 8 * (job.C * int(off[b]) + c * n)
        first += nb
    raise AssertionError(u)


def test_uniform_rows_are_whole_rows_at_their_addresses(tmp_path):
    job = make_job([300] * 10, batch=4)
    assert job.resident
    bench.dump_dsp(job, str(tmp_path), "envelopes", "", 1 << 20)
    env, idx = np.load(tmp_path / "envelopes.npy"), np.load(tmp_path / "envelopes_index.npy")
    assert env.dtype == idx.dtype == np.float64 and env.shape == (40, 300) and idx.shape == (40, 2)   # 10 x 4 rows < 256
    assert len(np.unique(idx, axis=0)) == 40
    for row, (u, c) in zip(env, idx.astype(int)):
        assert row[0] == expected_start(job, u, c) and np.all(np.diff(row) == 8)
    assert sorted(f.name for f in tmp_path.iterdir()) == ["envelopes.npy", "envelopes_index.npy"]


def test_sample_is_seeded_and_capped_by_the_budget(tmp_path):
    job = make_job([1000] * 100, batch=50, C=8)
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir()
    b.mkdir()
    bench.dump_dsp(job, str(a), "envelopes", "", 1 << 20)
    bench.dump_dsp(job, str(b), "envelopes", "", 1 << 20)
    ia, ib = np.load(a / "envelopes_index.npy"), np.load(b / "envelopes_index.npy")
    assert np.array_equal(ia, ib) and len(ia) == (1 << 20) // 8000        # 131 rows of 8000 B fit 1 MiB
    assert np.load(a / "envelopes.npy").nbytes <= 1 << 20
    full = tmp_path / "c"
    full.mkdir()
    bench.dump_dsp(job, str(full), "envelopes", "", bench.DUMP_BUDGET_BYTES)
    assert len(np.load(full / "envelopes_index.npy")) == bench.DUMP_MAX_ROWS


def test_ragged_rows_and_a_shared_output_region(tmp_path):
    """Ragged utterances: rows concatenated + their lengths. Batches that share one output region: only the last batch's
    rows survive the last step, and only they are sampled."""
    lens = [100, 200, 150, 120, 130]
    job = make_job(lens, batch=2, budget=1000)
    assert not job.resident and [nb for _, _, nb in job.batches] == [1, 2, 2]
    bench.dump_dsp(job, str(tmp_path), "envelopes", "_rank1", 1 << 20)
    env = np.load(tmp_path / "envelopes_rank1.npy")
    idx = np.load(tmp_path / "envelopes_index_rank1.npy").astype(int)
    n = np.load(tmp_path / "envelopes_lengths_rank1.npy").astype(int)
    assert set(idx[:, 0]) == {3, 4} and len(idx) == 2 * job.C
    assert np.array_equal(n, [lens[u] for u in idx[:, 0]]) and env.size == n.sum()
    starts = np.concatenate([[0], np.cumsum(n)[:-1]])
    for s, (u, c) in zip(starts, idx):
        assert env[s] == expected_start(job, u, c)


@pytest.mark.parametrize("n,budget,kept", [(100, 1 << 20, 100), (100000, 120000, 10000)])
def test_cnn_outputs_as_float32(tmp_path, n, budget, kept):
    dev = FakeDevice()
    d_scores, d_labels = dev.malloc(8 * n), dev.malloc(n)

    def d2h(arr, p):
        assert p in (d_scores, d_labels) and arr.nbytes == (8 * n if p == d_scores else n)
        arr.reshape(-1)[:] = np.arange(arr.size) % 2
    dev.d2h = d2h
    bench.dump_cnn(dev, d_scores, d_labels, n, str(tmp_path), "", budget)
    s, lab = np.load(tmp_path / "cnn_scores.npy"), np.load(tmp_path / "cnn_labels.npy")
    assert s.dtype == lab.dtype == np.float32 and s.shape == (kept, 2) and lab.shape == (kept,)
    assert (tmp_path / "cnn_index.npy").exists() == (kept < n)
